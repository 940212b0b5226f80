// map_file.h — the canonical file of a voxel map's exact state (include/wildcat_hip.h: wc_map_export_state / wc_map_absorb).
// Plain C++17: no HIP, no other header of the project.  Bytes in, bytes out, little-endian whatever the host.
//
//   header, 64 bytes   magic "WCMAPST1" | u32 version = 1 | u32 flags (bit 0: moments) | f64 voxel | u64 n | u64 points (= sum of the
//                      counts) | u64 FNV-1a-64 of the payload bytes | 16 zero bytes
//   payload            n records of 40 bytes (i32 key[3], u32 count, i64 sum[3]), then - bit 0 - n x 9 i64 moment words
//
// The keys ascend strictly in (kx, ky, kz), so one map has one byte string.  Decode refuses everything else, each reason with a code
// of its own, and reads no byte beyond `len` for any input.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace wc_map_file {

enum : int {
  kOk = 0,
  kBadMagic = 1,
  kBadVersion = 2,
  kBadFlags = 3,     // a flag bit this version does not know
  kBadReserved = 4,  // a non-zero reserved byte
  kBadVoxel = 5,     // outside [0.01, 4.0], or NaN
  kBadLength = 6,    // len != 64 + n * 40 (+ n * 72); a buffer shorter than the header
  kBadChecksum = 7,
  kBadPoints = 8,    // the header's points != the sum of the counts
  kBadRecord = 9,    // a record wc_map_absorb would reject: |key| >= 2^20 on an axis, count == 0 or count > 2^30
  kBadOrder = 10,    // keys not strictly ascending (a duplicate key included)
};

constexpr size_t kHeaderBytes = 64, kRecordBytes = 40, kMomentBytes = 72;
constexpr uint32_t kVersion = 1, kFlagMoments = 1;
constexpr char kMagic[9] = "WCMAPST1";

// the record as the library's wc_map_voxel lays it out (the facade asserts that the two agree)
struct Voxel {
  int32_t key[3];
  uint32_t count;
  int64_t sum[3];
};
static_assert(sizeof(Voxel) == kRecordBytes, "a state record is 40 bytes");

struct Header {
  uint32_t flags = 0;
  double voxel = 0;
  uint64_t n = 0, points = 0;
};

inline void PutU32(uint8_t *p, uint32_t x) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(x >> (8 * i));
}
inline void PutU64(uint8_t *p, uint64_t x) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(x >> (8 * i));
}
inline uint32_t GetU32(const uint8_t *p) {
  uint32_t x = 0;
  for (int i = 0; i < 4; ++i) x |= (uint32_t)p[i] << (8 * i);
  return x;
}
inline uint64_t GetU64(const uint8_t *p) {
  uint64_t x = 0;
  for (int i = 0; i < 8; ++i) x |= (uint64_t)p[i] << (8 * i);
  return x;
}
inline uint64_t Fnv1a64(const uint8_t *p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

inline size_t EncodedBytes(uint64_t n, bool moments) { return kHeaderBytes + (size_t)n * (kRecordBytes + (moments ? kMomentBytes : 0)); }

// the file of n records (mom: n x 9 words, looked at only with the moments flag) into out[EncodedBytes(n, moments)].  Nothing is
// validated here: a state Decode would refuse encodes to a file Decode refuses
inline void Encode(double voxel, uint32_t flags, const Voxel *vox, const int64_t *mom, uint64_t n, uint8_t *out) {
  const bool moments = (flags & kFlagMoments) != 0;
  uint8_t *pay = out + kHeaderBytes, *p = pay;
  uint64_t points = 0;
  for (uint64_t i = 0; i < n; ++i, p += kRecordBytes) {
    for (int a = 0; a < 3; ++a) PutU32(p + 4 * a, (uint32_t)vox[i].key[a]);
    PutU32(p + 12, vox[i].count);
    for (int a = 0; a < 3; ++a) PutU64(p + 16 + 8 * a, (uint64_t)vox[i].sum[a]);
    points += vox[i].count;
  }
  if (moments)
    for (uint64_t j = 0; j < 9 * n; ++j, p += 8) PutU64(p, (uint64_t)mom[j]);
  std::memcpy(out, kMagic, 8);
  PutU32(out + 8, kVersion);
  PutU32(out + 12, flags);
  uint64_t vbits;
  std::memcpy(&vbits, &voxel, 8);
  PutU64(out + 16, vbits);
  PutU64(out + 24, n);
  PutU64(out + 32, points);
  PutU64(out + 40, Fnv1a64(pay, (size_t)(p - pay)));
  std::memset(out + 48, 0, 16);
}

// kOk: buf[0, len) is a canonical state file and *h (may be null) describes it; anything else: the first reason found, in this order:
// a buffer shorter than the header, magic, version, flags, reserved bytes, voxel, length, checksum, then record by record its own
// fields before its place in the order, and the points sum last
inline int Decode(const uint8_t *buf, size_t len, Header *h) {
  if (!buf || len < kHeaderBytes) return kBadLength;
  if (std::memcmp(buf, kMagic, 8) != 0) return kBadMagic;
  if (GetU32(buf + 8) != kVersion) return kBadVersion;
  const uint32_t flags = GetU32(buf + 12);
  if (flags & ~kFlagMoments) return kBadFlags;
  for (size_t i = 48; i < kHeaderBytes; ++i)
    if (buf[i]) return kBadReserved;
  const uint64_t vbits = GetU64(buf + 16);
  double voxel;
  std::memcpy(&voxel, &vbits, 8);
  if (!(voxel >= 0.01 && voxel <= 4.0)) return kBadVoxel;
  const uint64_t n = GetU64(buf + 24), per = kRecordBytes + ((flags & kFlagMoments) ? kMomentBytes : 0);
  const size_t body = len - kHeaderBytes;
  if (n > body / per || n * per != body) return kBadLength;  // (n <= body / per first: the product cannot wrap)
  const uint8_t *pay = buf + kHeaderBytes;
  if (GetU64(buf + 40) != Fnv1a64(pay, body)) return kBadChecksum;
  uint64_t points = 0;
  int64_t prev[3] = {0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t *p = pay + i * kRecordBytes;
    int64_t k[3];
    for (int a = 0; a < 3; ++a) {
      k[a] = (int32_t)GetU32(p + 4 * a);
      if (k[a] <= -(1 << 20) || k[a] >= (1 << 20)) return kBadRecord;
    }
    const uint32_t count = GetU32(p + 12);
    if (count == 0 || count > (1u << 30)) return kBadRecord;
    if (i) {
      const bool above = k[0] != prev[0] ? k[0] > prev[0] : (k[1] != prev[1] ? k[1] > prev[1] : k[2] > prev[2]);
      if (!above) return kBadOrder;
    }
    for (int a = 0; a < 3; ++a) prev[a] = k[a];
    points += count;
  }
  if (points != GetU64(buf + 32)) return kBadPoints;
  if (h) h->flags = flags, h->voxel = voxel, h->n = n, h->points = points;
  return kOk;
}

// the records and moment words of a file Decode has accepted, into the host's own integers (mom: n x 9 words, may be null)
inline void Unpack(const uint8_t *buf, const Header &h, Voxel *vox, int64_t *mom) {
  const uint8_t *p = buf + kHeaderBytes;
  for (uint64_t i = 0; i < h.n; ++i, p += kRecordBytes) {
    for (int a = 0; a < 3; ++a) vox[i].key[a] = (int32_t)GetU32(p + 4 * a);
    vox[i].count = GetU32(p + 12);
    for (int a = 0; a < 3; ++a) vox[i].sum[a] = (int64_t)GetU64(p + 16 + 8 * a);
  }
  if (mom && (h.flags & kFlagMoments))
    for (uint64_t j = 0; j < 9 * h.n; ++j, p += 8) mom[j] = (int64_t)GetU64(p);
}

}  // namespace wc_map_file
