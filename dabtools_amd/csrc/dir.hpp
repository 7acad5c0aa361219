// dir.hpp — the ensemble directory: the device-side types of the kernels (k_dir.hip), shared with the host object (dir.cpp).  The rules are
// dir_figs.hpp's (free of HIP); dabhip.h has them in words; tests/dir_model.py restates them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "dir_figs.hpp"
#include "eti_push.hpp"

namespace dabhip {

// what the fibs kernel leaves per (stream, new frame, FIB) beside the FIB's fact slots; the frame's own class rides on its FIB 0
struct DirFib {
  uint8_t nfacts;
  uint8_t cls;                                           // kDirFib*
  uint8_t figs, truncated, ignored;
  uint8_t pad[3];
};
static_assert(sizeof(DirFib) == 8, "DirFib layout");
enum : int { kDirFibSeen = 1, kDirFibCrcFailed = 2, kDirFrame = 4, kDirFrameNoFic = 8, kDirFrameSkipped = 16 };

// One entry of a table: per part, the payload of the latest fact of that kind (dir_figs.hpp).  Parts: ensemble entries 0..3 = 0/0, 0/9, 0/10,
// label, each in part0; sub-channel: part0 = 0/1, part1 = 0/14; service: part0 = 0/2, part1 = label; packet component: part0 = 0/3.
struct DirEntry {
  uint32_t key;
  uint8_t pd;
  uint8_t have;                                          // bit p: part p holds a fact
  uint8_t pad[2];
  uint8_t part0[32];
  uint8_t part1[24];
  int64_t first, last, changes;
};
static_assert(sizeof(DirEntry) == 88, "DirEntry layout");

constexpr int kDirEnsEntries = 4;
constexpr int kDirSubBase = kDirEnsEntries, kDirSvcBase = kDirSubBase + kDirTable, kDirPktBase = kDirSvcBase + kDirTable;
constexpr int kDirEntries = kDirPktBase + kDirTable;     // 196

enum DirCounter : int {
  kDirCntFrames, kDirCntNoFic, kDirCntSkipped, kDirCntFibs, kDirCntCrcFailed, kDirCntFigs, kDirCntTruncated, kDirCntIgnored, kDirCntFacts, kDirCntChanged,
  kDirCntDropped, kDirCntN
};

// the state of one stream in device memory; reset clears `tables`: everything in front of `counters`
struct DirStream {
  DirEntry e[kDirEntries];
  int32_t nsvc, npkt;
  int64_t counters[kDirCntN];
};
constexpr size_t kDirTablesBytes = sizeof(DirEntry) * kDirEntries + 8;
static_assert(sizeof(DirStream) == kDirTablesBytes + 8 * kDirCntN && sizeof(DirStream) % 8 == 0, "DirStream layout");

}  // namespace dabhip
