"""CPU half of tests/test_window_params_gpu.py, nothing of the library involved: every case of tests/window_params_cases.py is LIVE on
each of its windows, and the two loss cases are the regimes they claim.

Live.  The oracle evaluated with the DEFAULT parameters on the case's window - what a device that ignored the parameter (200.0 for
1 / imu_dt, 0.16 for the loss, a weight left at its default or taken from another's place) would return - is held to the case's
reference (the short-sum reference under the case's parameters) with the case's bars: check_linearization's, floor and allowances of
the case, nothing widened.  It must leave the bar behind in every unknown-type pair the parameter reaches (window_params_cases.REACH),
at x = 0 and at the random point.  Measured excess over the bar (error / bar; the smallest over the reached pairs and both points):

    case                   default ns=8   six modes quirks=1   six modes quirks=0
    surfel_sigma0 0.05       2.7e+11          1.1e+11              1.1e+11
    surfel_sigma0 1e-3       2.6e+09          1.4e+09              1.4e+09
    cauchy_a 0.05            5.9e+09          2.5e+09              2.5e+09
    cauchy_a 50              3.5e+11          2.2e+11              2.2e+11
    imu_dt 0.0025            1.1e+08          5.3e+07              5.3e+07
    imu_dt 0.01              1.8e+08          1.2e+08              1.2e+08
    w_gyr x 3                1.6e+12          5.0e+11              1.4e+11
    w_acc / 3                9.5e+03          4.5e+03              4.5e+03
    w_bg x 3                 1.1e+13          1.1e+13              1.1e+13
    w_ba / 3                 1.0e+14          9.8e+13              9.8e+13
    everything together      3.3e+09          1.9e+09              1.9e+09

(w_acc / 3: the b2 x b2 pair, which the far larger w_ba terms share; its pos x b2 pair is 1e8 over.)  A run with -s prints the table.

Regimes.  From the oracle's own residuals at x = 0: with cauchy_a = 0.05 (b = 2.5e-3) r^2 > b for most surfel factors - 232 of 250 on
the 8-state window, 1128 of 1198 on the six-mode window -, with cauchy_a = 50 (b = 2500) for none of the matcher's correspondences
(largest |r| 1.5 on the 8-state window).  The six-mode window's hand-made Mode 2 pairs join two arbitrary surfels of one sample
interval, metres apart: 19 of them (|r| up to 625) lie past b = 2500 too, and nothing else does - the test asserts exactly that."""
import numpy as np
import pytest

import linearize_ref as lr
import window_params_cases as wp

TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    for name in wp.CASES:  # (shown by a run with -s)
        if all((w, name) in TABLE for w in wp.WINDOWS):
            print("    %-22s " % name + "   ".join("%.1e" % TABLE[(w, name)] for w in wp.WINDOWS))


@pytest.mark.parametrize("name", list(wp.CASES))
@pytest.mark.parametrize("which", wp.WINDOWS)
def test_case_is_live(oracle, which, name):
    sp0 = wp.window(oracle, which)
    sp = wp.with_case(oracle, sp0, name)
    assert bytes(sp["params"]) != bytes(sp0["params"])
    W0, W = lr.oracle_window(oracle, sp0), lr.oracle_window(oracle, sp)
    assert W0.counts() == W.counts()  # the same factors: only their parameters differ
    least = np.inf
    for x in wp.points(sp0):
        ref = lr.reference(oracle, sp, x)
        floor = lr.scaled_errors(*W.linearize(x), *ref)
        allow = lr.allowances(sp, x, ref[0], ref[2])
        assert lr.within(floor, floor, allow)  # the case's own oracle passes the case's bars ...
        e = lr.scaled_errors(*W0.linearize(x), *ref)
        assert not lr.within(e, floor, allow), (which, name)  # ... the default-parameter oracle does not,
        xH, _, _ = wp.excess(e, floor, allow)
        xH = np.maximum(xH, xH.T)
        for a, b in wp.REACH[name]:  # and that in every sub-block the parameter reaches
            assert xH[a, b] > 1.0, (which, name, lr.TYPES[a], lr.TYPES[b], xH[a, b])
            least = min(least, xH[a, b])
    TABLE[(which, name)] = least
    assert least > 1e3  # (none of the cases is live by a hair: the smallest measured is 4.5e3)


@pytest.mark.parametrize("which", wp.WINDOWS)
def test_the_two_loss_cases_are_the_regimes_they_claim(oracle, which):
    sp0 = wp.window(oracle, which)
    n_matched = len(sp0["pairs"]) - (0 if which == "default ns=8" else _hand_made(sp0))
    past = {}
    for name in ("cauchy_a 0.05", "cauchy_a 50"):
        sp = wp.with_case(oracle, sp0, name)
        W = lr.oracle_window(oracle, sp)
        _, res = W.evaluate(np.zeros(12 * W.ns), want_residuals=True)
        c = W.counts()
        n = len(res) - 12 * (c[4] + c[5])
        assert n == len(sp0["pairs"]) + len(sp0["pf"])
        past[name] = np.nonzero(wp.raw_r2(res[:n], sp["params"].cauchy_a) > sp["params"].cauchy_a ** 2)[0]
        print("%s %s: r^2 > b for %d of %d surfel factors" % (which, name, len(past[name]), n))
    assert len(past["cauchy_a 0.05"]) > 0.9 * n  # deep in the tail: most factors
    hand_made = (past["cauchy_a 50"] >= n_matched) & (past["cauchy_a 50"] < len(sp0["pairs"]))
    assert np.all(hand_made) and (which != "default ns=8" or len(past["cauchy_a 50"]) == 0)  # no factor of a matched correspondence reaches it
    assert len(past["cauchy_a 50"]) <= 25


def _hand_made(sp0):
    """the number of hand-made Mode 2 pairs at the end of the six-mode window's binary list (test_window_gpu._mode2_pairs)"""
    from test_window_gpu import _mode2_pairs

    return len(_mode2_pairs(sp0["w"], 25, np.random.default_rng(11)))
