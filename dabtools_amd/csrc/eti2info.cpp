// eti2info.cpp — what an ensemble carries: reads ETI(NI) frames from stdin, builds the ensemble directory on the GPU (dabhip_dir_*) and prints it
//   dab2eti-hip capture.cu8 | eti2info [--first-complete] [--json]
// One block on stdout when stdin ends, or with --first-complete as soon as the directory is complete: the ensemble, a line per sub-channel, a
// line per service and per component with its kind, and for every component that resolves the command that extracts it.  Label bytes
// 0x20..0x7E are printed as they are and every other byte as \xHH, the charset number beside; a full EBU Latin table is out of scope.  --json
// prints the same as one JSON object, labels as hex.  The eleven counters go to stderr as one line.  Exit status 0, or 3 when the input ended
// before the directory was complete.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "eti_stdin.hpp"

namespace {
const char* const kKinds[] = {"unknown", "mp2", "dabplus", "ts", "stream-data", "packet"};

std::string label_text(const uint8_t* l)
{
  std::string s;
  char buf[8];
  for (int i = 0; i < 16; ++i) {
    if (l[i] >= 0x20 && l[i] <= 0x7e && l[i] != '\\') s += static_cast<char>(l[i]);
    else { std::snprintf(buf, sizeof buf, "\\x%02X", l[i]); s += buf; }
  }
  return s;
}
std::string label_hex(const uint8_t* l)
{
  std::string s;
  char buf[4];
  for (int i = 0; i < 16; ++i) { std::snprintf(buf, sizeof buf, "%02x", l[i]); s += buf; }
  return s;
}
std::string command(const dabhip_dir_target& t)
{
  char buf[96];
  switch (t.kind) {
    case DABHIP_DIR_MP2: std::snprintf(buf, sizeof buf, "eti2mpa %d", t.subch); break;
    case DABHIP_DIR_DABPLUS: std::snprintf(buf, sizeof buf, "eti2aac %d", t.subch); break;
    case DABHIP_DIR_TS: std::snprintf(buf, sizeof buf, "eti2ts %d", t.subch); break;
    case DABHIP_DIR_PACKET: std::snprintf(buf, sizeof buf, "eti2pkt %d%s --address %d", t.subch, t.fec ? " --fec" : "", t.address); break;
    default: return "";
  }
  return buf;
}
const char* prot_text(const dabhip_dir_subch& s, char* buf, size_t n)
{
  if (!(s.have & DABHIP_DIR_SUB_HAVE_01)) std::snprintf(buf, n, "-");
  else if (!s.form) std::snprintf(buf, n, "UEP %d", s.protlev);
  else std::snprintf(buf, n, "EEP %d-%c", (s.protlev & 3) + 1, (s.protlev & 4) ? 'B' : 'A');
  return buf;
}
}  // namespace

int main(int argc, char** argv)
{
  bool first_complete = false, json = false, bad = false;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--first-complete")) first_complete = true;
    else if (!std::strcmp(argv[i], "--json")) json = true;
    else bad = true;
  }
  if (bad) {
    std::fprintf(stderr, "Usage: eti2info [--first-complete] [--json]   (ETI on stdin; the ensemble's services, components and sub-channels on stdout.\n"
                         "  Labels: bytes 0x20..0x7E as they are, others as \\xHH, with the charset number; no EBU Latin table.)\n");
    return 1;
  }
  dabhip_dir* d = dabhip_dir_create(0, 1);
  if (!d) { std::fprintf(stderr, "eti2info: %s\n", dabhip_last_error()); return 2; }
  int complete = 0;
  int rc = for_eti_frames(0, 4, [&](const uint8_t* f, int64_t n) {
    if (dabhip_dir_push(d, f, &n, 0) < 0) { std::fprintf(stderr, "eti2info: %s\n", dabhip_last_error()); return 2; }
    return first_complete && dabhip_dir_complete(d, 0) != 0 ? -1 : 0;      // seen enough
  });
  if (rc == 0) {
    complete = dabhip_dir_complete(d, 0);
    if (complete < 0) { std::fprintf(stderr, "eti2info: %s\n", dabhip_last_error()); rc = 2; }
  }
  if (rc == 0) {
    dabhip_dir_ensemble_rec e;
    std::vector<dabhip_dir_subch> sub(64);
    std::vector<dabhip_dir_service> svc(64);
    std::vector<dabhip_dir_pktcomp> pkt(64);
    dabhip_dir_ensemble(d, 0, &e);
    sub.resize(static_cast<size_t>(dabhip_dir_subchannels(d, 0, sub.data(), 64)));
    svc.resize(static_cast<size_t>(dabhip_dir_services(d, 0, svc.data(), 64)));
    pkt.resize(static_cast<size_t>(dabhip_dir_packet_components(d, 0, pkt.data(), 64)));
    char pb[32];
    if (!json) {
      std::printf("ensemble EId 0x%04X ECC 0x%02X label \"%s\" charset %d", e.eid, e.ecc, (e.have & DABHIP_DIR_HAVE_LABEL) ? label_text(e.label).c_str() : "", e.charset);
      if (e.have & DABHIP_DIR_HAVE_10) std::printf(" time MJD %u %02d:%02d:%02d.%03d UTC (frame %lld)", e.mjd, e.hours, e.minutes, e.seconds, e.milliseconds, static_cast<long long>(e.time_frame));
      std::printf("%s\n", complete ? "" : " (incomplete)");
      for (const dabhip_dir_subch& s : sub)
        std::printf("subch %2d start %3d size %3d %s %3d kbit/s fec-scheme %d\n", s.id, s.start_cu, s.size_cu, prot_text(s, pb, sizeof pb), s.bitrate, s.fec_scheme);
    } else {
      std::printf("{\"complete\": %s, \"ensemble\": {\"eid\": %d, \"ecc\": %d, \"label\": \"%s\", \"charset\": %d, \"have\": %d, \"mjd\": %u, \"hours\": %d, \"minutes\": %d, "
                  "\"seconds\": %d, \"milliseconds\": %d, \"time_frame\": %lld}, \"subchannels\": [",
                  complete ? "true" : "false", e.eid, e.ecc, label_hex(e.label).c_str(), e.charset, e.have, e.mjd, e.hours, e.minutes, e.seconds, e.milliseconds,
                  static_cast<long long>(e.time_frame));
      for (size_t i = 0; i < sub.size(); ++i)
        std::printf("%s{\"id\": %d, \"start\": %d, \"size\": %d, \"form\": %d, \"protlev\": %d, \"bitrate\": %d, \"fec_scheme\": %d}", i ? ", " : "", sub[i].id,
                    sub[i].start_cu, sub[i].size_cu, sub[i].form, sub[i].protlev, sub[i].bitrate, sub[i].fec_scheme);
      std::printf("], \"services\": [");
    }
    for (size_t i = 0; i < svc.size(); ++i) {
      const dabhip_dir_service& s = svc[i];
      if (!json) std::printf("service %s 0x%0*X label \"%s\" charset %d components %d\n", s.pd ? "data" : "programme", s.pd ? 8 : 4, s.sid,
                             (s.have & DABHIP_DIR_SVC_HAVE_LABEL) ? label_text(s.label).c_str() : "", s.charset, s.ncomp);
      else std::printf("%s{\"pd\": %d, \"sid\": %u, \"label\": \"%s\", \"charset\": %d, \"components\": [", i ? ", " : "", s.pd, s.sid, label_hex(s.label).c_str(), s.charset);
      for (int c = 0; c < s.ncomp; ++c) {
        dabhip_dir_target t;
        const int r = dabhip_dir_resolve(d, 0, s.pd, s.sid, c, &t);
        const int tmid = s.comp[2 * c] >> 6;
        const std::string cmd = r == 0 ? command(t) : "";
        if (!json) {
          if (r != 0) std::printf("  component %d TMId %d: unresolved (%s)\n", c, tmid, dabhip_last_error());
          else if (t.kind == DABHIP_DIR_PACKET) std::printf("  component %d %s subch %d SCId %d address %d DSCTy %d DG-flag %d%s: %s\n", c, kKinds[t.kind], t.subch, t.scid, t.address, t.dscty,
                                                            t.dg, t.fec ? " fec" : "", cmd.c_str());
          else std::printf("  component %d %s subch %d%s%s\n", c, kKinds[t.kind], t.subch, cmd.empty() ? "" : ": ", cmd.c_str());
        } else {
          std::printf("%s{\"tmid\": %d, \"resolved\": %s, \"kind\": \"%s\", \"subch\": %d, \"address\": %d, \"fec\": %d, \"command\": \"%s\"}", c ? ", " : "", tmid,
                      r == 0 ? "true" : "false", r == 0 ? kKinds[t.kind] : "", r == 0 ? t.subch : -1, r == 0 ? t.address : 0, r == 0 ? t.fec : 0, cmd.c_str());
        }
      }
      if (json) std::printf("]}");
    }
    if (json) std::printf("]}\n");
    std::fflush(stdout);
  }
  int64_t c[11] = {0};
  dabhip_dir_stats(d, 0, c);
  std::fprintf(stderr, "eti2info: %lld frames (%lld without FIC, %lld skipped), %lld FIBs (%lld CRC failed), %lld FIGs (%lld truncated, %lld ignored), %lld facts "
               "(%lld changed, %lld dropped)\n",
               static_cast<long long>(c[0]), static_cast<long long>(c[1]), static_cast<long long>(c[2]), static_cast<long long>(c[3]), static_cast<long long>(c[4]),
               static_cast<long long>(c[5]), static_cast<long long>(c[6]), static_cast<long long>(c[7]), static_cast<long long>(c[8]), static_cast<long long>(c[9]),
               static_cast<long long>(c[10]));
  dabhip_dir_destroy(d);
  if (rc == 0 && !complete) rc = 3;
  return rc;
}
