// map_room.h — the voxel map's room policy: what precedes every call that may create up to n voxels.  Plain C++17, no HIP
// and no other project header: csrc/map.hip acts on the decision, the facade library exports it as wc_host_map_room for the tests.
//
// The table (open addressing, a power-of-two number of slots) is at most half full at every probe.  A removed voxel leaves a tombstone
// (map.hip: kMapTomb) that holds its slot until the table is replaced, so the slots in use are the live voxels AND the tombstones.
#pragma once
#include <cstdint>

enum : int { kMapRoomKeep = 0, kMapRoomGrow = 1, kMapRoomPurge = 2, kMapRoomFull = -1 };
constexpr uint64_t kMapRoomMaxCap = (uint64_t)1 << 32;  // slots

inline uint64_t pow2_at_least(uint64_t x) {
  uint64_t c = 1;
  while (c < x) c <<= 1;
  return c;
}

// cap: the table's slots; live_bound: an upper bound of its live voxels; tombs: its tombstones (exact); n: the voxels the call may create.
//   2 (live_bound + tombs + n) <= cap   kMapRoomKeep: the table stays, *new_cap = cap
//   otherwise *new_cap = max(cap, pow2_at_least(2 (live_bound + n))): a replacement never shrinks the table and drops every tombstone;
//   equal to cap: kMapRoomPurge (a fresh table of the same size); larger: kMapRoomGrow; beyond 2^32 slots: kMapRoomFull, *new_cap = cap
// With tombs = 0 this is the growth policy as it was before voxels could be removed.
inline int map_room(uint64_t cap, uint64_t live_bound, uint64_t tombs, uint64_t n, uint64_t *new_cap) {
  *new_cap = cap;
  const uint64_t need = 2 * (live_bound + n);
  if (need + 2 * tombs <= cap) return kMapRoomKeep;
  if (need > kMapRoomMaxCap) return kMapRoomFull;  // (pow2_at_least(need) would exceed 2^32)
  const uint64_t want = pow2_at_least(need);
  if (want <= cap) return kMapRoomPurge;
  *new_cap = want;
  return kMapRoomGrow;
}
