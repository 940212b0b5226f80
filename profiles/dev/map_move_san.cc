// map_move_san.cc - a stand-alone program (its own main, no GPU, no Python) that runs wc_map_move_state, the host entry point of the
// per-voxel move (csrc/map.hip: map_move_voxel), under AddressSanitizer and UBSan on the host: the records of a state
// file, then batches of random records - keys over and beyond the range, counts of 0 .. 2^30 + 1, sums and moment words of any 64-bit
// value, which no insert could have produced - under random rigid poses with translations up to the end of the key range, every input
// and output in a heap block of exactly its length.  Prints how many records were moved and how many rejected.
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//     -I include -I wildcat-slam_amd/host wildcat-slam_amd/csrc/*.hip profiles/dev/map_move_san.cc -ldl -pthread -o /tmp/map_move_san
//   /tmp/map_move_san tests/golden/map_state_v1.bin
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "map_file.h"
#include "wildcat_hip.h"

static void Pose(std::mt19937_64 &rng, double reach, double T[12]) {
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  double q[4], n = 0;
  for (double &x : q) x = u(rng), n += x * x;
  n = std::sqrt(n);
  for (double &x : q) x /= n;
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = reach * u(rng);
  }
}

// one call on heap blocks of exactly the lengths given -> records rejected
static uint64_t Move(const std::vector<wc_map_voxel> &vox, const std::vector<int64_t> &mom, bool moments, double voxel, const double T[12]) {
  const size_t n = vox.size();
  const size_t vb = n ? n * sizeof(wc_map_voxel) : 1, mb = n ? n * 72 : 1;  // (n = 0: one byte nobody may touch)
  wc_map_voxel *in = (wc_map_voxel *)std::malloc(vb), *out = (wc_map_voxel *)std::malloc(vb);
  int64_t *im = moments ? (int64_t *)std::malloc(mb) : nullptr, *om = moments ? (int64_t *)std::malloc(mb) : nullptr;
  if (n) std::memcpy(in, vox.data(), n * sizeof(wc_map_voxel));
  if (n && moments) std::memcpy(im, mom.data(), n * 72);
  uint64_t rej = 0;
  if (wc_map_move_state(in, im, n, voxel, T, out, om, &rej) != WC_OK) std::abort();
  uint64_t zero = 0;
  for (size_t i = 0; i < n; ++i) zero += out[i].count == 0;
  if (zero != rej) std::abort();  // (a rejected record is written as count 0, and only a rejected one)
  std::free(in), std::free(out), std::free(im), std::free(om);
  return rej;
}

int main(int argc, char **argv) {
  if (argc < 2) return 3;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<uint8_t> file(1 << 20);
  file.resize(std::fread(file.data(), 1, file.size(), f));
  std::fclose(f);
  wc_map_file::Header h;
  if (wc_map_file::Decode(file.data(), file.size(), &h) != wc_map_file::kOk) return 4;
  std::vector<wc_map_file::Voxel> fv(h.n);
  std::vector<int64_t> fm(9 * h.n);
  wc_map_file::Unpack(file.data(), h, fv.data(), fm.data());
  std::vector<wc_map_voxel> vox(h.n);
  std::memcpy(vox.data(), fv.data(), h.n * sizeof(wc_map_voxel));
  std::mt19937_64 rng(12345);
  uint64_t moved = 0, rejected = 0;
  for (int rep = 0; rep < 1000; ++rep) {
    double T[12];
    Pose(rng, rep % 2 ? 1.0 : 3e5, T);
    const uint64_t r = Move(vox, fm, rep % 3 != 0, h.voxel, T);
    rejected += r, moved += h.n - r;
  }
  const double sizes[] = {0.01, 0.05, 0.2, 0.8, 2.0, 2.5, 4.0};
  for (int rep = 0; rep < 2000; ++rep) {
    const size_t n = rng() % 300;
    const double v = sizes[rng() % 7];
    std::vector<wc_map_voxel> rv(n);
    std::vector<int64_t> rm(9 * n);
    for (size_t i = 0; i < n; ++i) {
      for (int a = 0; a < 3; ++a) {
        rv[i].key[a] = rng() % 16 ? (int32_t)(rng() % (1u << 21)) - (1 << 20) : (int32_t)rng();
        rv[i].sum[a] = rng() % 4 ? (int64_t)(rng() >> (1 + rng() % 63)) * (rng() % 2 ? 1 : -1) : (int64_t)rng();
      }
      rv[i].count = rng() % 8 ? (uint32_t)(rng() % 1000) : (uint32_t)(rng() % ((1u << 30) + 2));
      for (int w = 0; w < 9; ++w) rm[9 * i + w] = rng() % 4 ? (int64_t)(rng() >> (1 + rng() % 63)) * (rng() % 2 ? 1 : -1) : (int64_t)rng();
    }
    double T[12];
    Pose(rng, rep % 2 ? 10.0 : 1e6 * v, T);
    const uint64_t r = Move(rv, rm, rep % 3 != 0, v, T);
    rejected += r, moved += n - r;
  }
  std::printf("moved %llu records, rejected %llu: clean\n", (unsigned long long)moved, (unsigned long long)rejected);
  return 0;
}
