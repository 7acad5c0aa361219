// packet.hpp — packet-mode data sub-channels (ETSI EN 300 401 clauses 5.3.2, 5.3.3, 5.3.5): the device-side types of the kernels (k_packet.hip),
// shared with the host object (packet.cpp).  The sizes, the header rules and the sync rule are in packet_sync.hpp (free of HIP); dabhip.h has
// the rules in words; the plain-numpy restatement of all of it is tests/packet_model.py.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "eti_push.hpp"
#include "packet_sync.hpp"

namespace dabhip {

// ---- device-side records of k_packet.hip -------------------------------------------------------------------------------------------------------
// where one requested sub-channel sits in one new ETI frame of the push: [stream][frame][sub]
struct PacketLoc {
  const uint8_t* ptr;                       // first payload byte; null: absent, STL 0 or not a multiple of 3, or past the frame
  int32_t stl;
  int32_t cell0;                            // the lane's virtual index of its first cell (layout pass of the sync kernel)
};
static_assert(sizeof(PacketLoc) == 16, "PacketLoc layout");

// a unit in its lane's slot (sync kernel) and in the push's list (jobs kernel): its first cell in the lane's virtual numbering, the cells walked
// (94, or s without FEC), the cells held in the cell buffer (103, or s)
struct PacketSlot {
  int32_t u0;
  int16_t ncells;
  int16_t flags;                            // DABHIP_PACKET_FROM_FEC / _FROM_MISS
  int64_t cell_index;                       // of its first cell, since creation
};
struct PacketUnit {
  int32_t lane, u0;
  int32_t ncells, nbuf;
  int32_t flags;
  int32_t buf0;                             // its first cell in the cell buffer
  int64_t cell_index;
};
static_assert(sizeof(PacketSlot) == 16 && sizeof(PacketUnit) == 32, "packet unit layout");

enum PacketCounter : int { kPkCntFrames, kPkCntMisses, kPkCntSyncLosses, kPkCntSkipped, kPkCntBadCells, kPkCntPackets, kPkCntRsCorrected, kPkCntRsFailed, kPkCntN = 8 };

}  // namespace dabhip
