// eti2pkt.cpp — the packet-mode counterpart of eti2aac: reads ETI(NI) frames from stdin and writes the MSC data groups of one packet-mode
// sub-channel on stdout
//   dab2eti-hip capture.cu8 | eti2pkt N [--fec] [--address A] > groups.bin
// Cell sync, RS(204,188) correction (--fec: the sub-channel carries the enhanced packet mode's FEC frames) and the packet CRCs run on the GPU
// (dabhip_packet_*); the data groups are put together on the host (dabhip_packet_groups_*).  Whatever whole frames are on hand after each read
// are pushed at once, so a live pipe keeps its latency.  Every complete data group whose CRC is good or absent is written as its address (2
// bytes, most significant first), its length (2 bytes) and its bytes; --address keeps one address only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"
#include "eti_stdin.hpp"

int main(int argc, char** argv)
{
  int want = -1, address = -1;
  uint8_t fec = 0;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--fec")) fec = 1;
    else if (!std::strcmp(argv[i], "--address") && i + 1 < argc) address = std::atoi(argv[++i]);
    else want = std::atoi(argv[i]);
  }
  if (want < 0 || want > 63 || address > 1023) {
    std::fprintf(stderr, "Usage: eti2pkt N [--fec] [--address A]   (N = packet-mode sub-channel id; ETI on stdin, data groups on stdout)\n");
    return 1;
  }
  const int32_t id = want;
  dabhip_packet* d = dabhip_packet_create(0, 1, &id, &fec, 1);
  if (!d) { std::fprintf(stderr, "eti2pkt: %s\n", dabhip_last_error()); return 2; }
  dabhip_packet_groups* g = dabhip_packet_groups_create();
  std::vector<uint8_t> data, group;
  std::vector<dabhip_packet_rec> recs;
  long frames = 0, written = 0;
  const auto failed = [] { std::fprintf(stderr, "eti2pkt: %s\n", dabhip_last_error()); return 2; };
  const int rc = for_eti_frames(0, 3, [&](const uint8_t* f, int64_t n) {
    if (dabhip_packet_push(d, f, &n, 0) < 0) return failed();
    frames += n;
    const int64_t np = dabhip_packet_records(d, 0, 0, nullptr, 0);
    const int64_t nb = dabhip_packet_data(d, 0, 0, nullptr, 0);
    if (np < 0 || nb < 0) return failed();
    recs.resize(static_cast<size_t>(np));
    data.resize(static_cast<size_t>(nb));
    if (dabhip_packet_records(d, 0, 0, recs.data(), np) != np || dabhip_packet_data(d, 0, 0, data.data(), nb) != nb) return failed();
    const int64_t ng = dabhip_packet_groups_push(g, recs.data(), np, data.data(), nb);
    if (ng < 0) return failed();
    bool good = true;
    for (int64_t i = 0; i < ng && good; ++i) {
      dabhip_packet_group rec;
      const int64_t len = dabhip_packet_groups_get(g, i, &rec, nullptr, 0);
      if (len < 0 || (rec.crc_flag && !rec.crc_ok) || (address >= 0 && rec.address != address)) continue;
      group.resize(static_cast<size_t>(len) + 4);
      group[0] = static_cast<uint8_t>(rec.address >> 8);
      group[1] = static_cast<uint8_t>(rec.address & 0xff);
      group[2] = static_cast<uint8_t>(len >> 8);
      group[3] = static_cast<uint8_t>(len & 0xff);
      dabhip_packet_groups_get(g, i, nullptr, group.data() + 4, len);
      good = write_all(group.data(), group.size());
      ++written;
    }
    return good ? 0 : 3;
  });
  int64_t c[8] = {0}, gc[4] = {0};
  dabhip_packet_stats(d, 0, 0, c);
  dabhip_packet_groups_stats(g, gc);
  std::fprintf(stderr, "eti2pkt: %ld frames, sub-channel %d: %lld units, %lld missed frames, %lld sync losses, %lld cells skipped, %lld bad cells, %lld packets, "
               "%lld RS corrected bytes, %lld RS failed code words; %lld data groups (%ld written), %lld dropped, %lld orphan packets, %lld CRC fails\n",
               frames, want, static_cast<long long>(c[0]), static_cast<long long>(c[1]), static_cast<long long>(c[2]), static_cast<long long>(c[3]),
               static_cast<long long>(c[4]), static_cast<long long>(c[5]), static_cast<long long>(c[6]), static_cast<long long>(c[7]),
               static_cast<long long>(gc[0]), written, static_cast<long long>(gc[1]), static_cast<long long>(gc[2]), static_cast<long long>(gc[3]));
  dabhip_packet_groups_destroy(g);
  dabhip_packet_destroy(d);
  return rc;
}
