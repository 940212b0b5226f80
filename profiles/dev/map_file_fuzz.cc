// map_file_fuzz.cc - a stand-alone program (no GPU, no Python) that runs host/map_file.h's decoder under AddressSanitizer and UBSan:
// every truncation of a state file, every single-bit flip and 200 000 random mutations of it (half of them with the checksum made right
// again, so that the record rules are reached), each handed to Decode in a heap block of exactly the length given; then decode, unpack
// and re-encode of the file itself.  Prints how often each return code came up.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I wildcat-slam_amd/host profiles/dev/map_file_fuzz.cc -o /tmp/map_file_fuzz
//   /tmp/map_file_fuzz tests/golden/map_state_v1.bin
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "map_file.h"

using namespace wc_map_file;

static int DecodeCopy(const std::vector<uint8_t> &d, size_t len, Header *h) {
  uint8_t *p = (uint8_t *)std::malloc(len ? len : 1);
  if (len) std::memcpy(p, d.data(), len);
  const int rc = Decode(p, len, h);
  if (rc == kOk) {
    std::vector<Voxel> v(h->n);
    std::vector<int64_t> m(9 * h->n);
    Unpack(p, *h, v.data(), m.data());
  }
  std::free(p);
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 2) return 3;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<uint8_t> d(1 << 20);
  d.resize(std::fread(d.data(), 1, d.size(), f));
  std::fclose(f);
  Header h;
  long counts[11] = {0};
  if (d.size() < kHeaderBytes || DecodeCopy(d, d.size(), &h) != kOk) return 1;
  for (size_t cut = 0; cut < d.size(); ++cut) counts[DecodeCopy(d, cut, &h)]++;
  for (size_t i = 0; i < d.size(); ++i)
    for (int b = 0; b < 8; ++b) {
      std::vector<uint8_t> e = d;
      e[i] ^= (uint8_t)(1 << b);
      counts[DecodeCopy(e, e.size(), &h)]++;
    }
  std::mt19937_64 rng(1);
  for (int it = 0; it < 200000; ++it) {
    std::vector<uint8_t> e = d;
    const int k = 1 + (int)(rng() % 4);
    for (int j = 0; j < k; ++j) e[rng() % e.size()] = (uint8_t)rng();
    if (rng() % 8 == 0) PutU64(e.data() + 24, rng() % 3 ? rng() : rng() % 16);  // n: anything, or something small
    if (rng() % 4 == 0) e.resize(rng() % (e.size() + 40));
    if (e.size() >= kHeaderBytes && rng() % 2) PutU64(e.data() + 40, Fnv1a64(e.data() + kHeaderBytes, e.size() - kHeaderBytes));
    counts[DecodeCopy(e, e.size(), &h)]++;
  }
  DecodeCopy(d, d.size(), &h);
  std::vector<Voxel> v(h.n);
  std::vector<int64_t> m(9 * h.n);
  Unpack(d.data(), h, v.data(), m.data());
  std::vector<uint8_t> o(EncodedBytes(h.n, (h.flags & kFlagMoments) != 0));
  Encode(h.voxel, h.flags, v.data(), m.data(), h.n, o.data());
  if (o != d) return 2;
  for (int c = 0; c < 11; ++c) std::printf("code %d: %ld\n", c, counts[c]);
  return 0;
}
