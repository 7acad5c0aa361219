// packet_groups.hpp — the host rule that turns the packets of one packet-mode sub-channel into MSC data groups (ETSI EN 300 401 clauses 5.3.2.1
// and 5.3.3; dabhip.h: dabhip_packet_groups has it in words).  Host-only and free of HIP, so tests/host_sanitize/packet_units.cpp runs this text.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/dabhip.h"
#include "dab_bits.hpp"

namespace dabhip {

constexpr int kPkMaxGroup = 8208;

// the header fields of a complete group
inline dabhip_packet_group parse_group(int address, const std::vector<uint8_t>& b)
{
  dabhip_packet_group g;
  std::memset(&g, 0, sizeof g);
  g.address = address;
  g.length = static_cast<int32_t>(b.size());
  g.segment_number = g.transport_id = -1;
  if (b.size() < 2) return g;
  g.ext_flag = b[0] >> 7;
  g.crc_flag = (b[0] >> 6) & 1;
  g.seg_flag = (b[0] >> 5) & 1;
  g.ua_flag = (b[0] >> 4) & 1;
  g.type = b[0] & 15;
  g.continuity = b[1] >> 4;
  g.repetition = b[1] & 15;
  if (g.crc_flag && b.size() >= 4) {
    const uint16_t c = static_cast<uint16_t>(~crc16_ccitt(b.data(), b.size() - 2));
    g.crc_ok = c == ((b[b.size() - 2] << 8) | b[b.size() - 1]);
  }
  size_t at = 2;
  const size_t end = b.size() - (g.crc_flag ? 2 : 0);
  size_t need = at + (g.ext_flag ? 2 : 0) + (g.seg_flag ? 2 : 0) + (g.ua_flag ? 1 : 0);
  if (b.size() < (g.crc_flag ? 2u : 0u) || need > end) return g;
  uint16_t ext = 0;
  if (g.ext_flag) {
    ext = static_cast<uint16_t>((b[at] << 8) | b[at + 1]);
    at += 2;
  }
  int seg = -1, last = 0, tid = -1;
  if (g.seg_flag) {
    last = b[at] >> 7;
    seg = ((b[at] & 0x7f) << 8) | b[at + 1];
    at += 2;
  }
  if (g.ua_flag) {
    const int tflag = (b[at] >> 4) & 1, li = b[at] & 15;
    ++at;
    if (at + li > end || (tflag && li < 2)) return g;
    if (tflag) tid = (b[at] << 8) | b[at + 1];
  }
  g.header_ok = 1;
  g.ext_field = ext;
  g.last_segment = static_cast<uint8_t>(last);
  g.segment_number = seg;
  g.transport_id = tid;
  return g;
}

enum GroupCounter : int { kGrpDone, kGrpDropped, kGrpOrphans, kGrpCrcFails, kGrpN = 4 };

struct PacketGroups {
  struct Open {
    std::vector<uint8_t> bytes;
    int ci = 0;
  };
  std::map<int, Open> open;                          // by address
  std::vector<dabhip_packet_group> done;             // of the last push
  std::vector<std::vector<uint8_t>> done_bytes;
  int64_t counters[kGrpN] = {0, 0, 0, 0};

  // one packet (padding and command packets are passed over) with its useful bytes
  void packet(const dabhip_packet_rec& r, const uint8_t* useful)
  {
    if (r.address == 0 || r.command) return;
    const bool first = r.first_last & 2, last = r.first_last & 1;
    auto it = open.find(r.address);
    if (first) {
      if (it != open.end()) ++counters[kGrpDropped];
      else it = open.emplace(r.address, Open()).first;
      it->second.bytes.clear();
    } else {
      if (it == open.end()) {
        ++counters[kGrpOrphans];
        return;
      }
      if (((it->second.ci + 1) & 3) != r.continuity) {
        ++counters[kGrpDropped];
        open.erase(it);
        return;
      }
    }
    Open& o = it->second;
    o.ci = r.continuity;
    if (o.bytes.size() + r.useful_length > static_cast<size_t>(kPkMaxGroup)) {
      ++counters[kGrpDropped];
      open.erase(it);
      return;
    }
    o.bytes.insert(o.bytes.end(), useful, useful + r.useful_length);
    if (!last) return;
    const dabhip_packet_group g = parse_group(r.address, o.bytes);
    ++counters[kGrpDone];
    if (g.crc_flag && !g.crc_ok) ++counters[kGrpCrcFails];
    done.push_back(g);
    done_bytes.push_back(std::move(o.bytes));
    open.erase(it);
  }

  // the records of a push with their useful bytes one after another; false when the bytes run short
  bool push(const dabhip_packet_rec* recs, int64_t nrecs, const uint8_t* data, int64_t ndata)
  {
    done.clear();
    done_bytes.clear();
    int64_t at = 0;
    for (int64_t i = 0; i < nrecs; ++i) {
      if (at + recs[i].useful_length > ndata) return false;
      packet(recs[i], data + at);
      at += recs[i].useful_length;
    }
    return true;
  }
};

}  // namespace dabhip
