// edirx_units.cpp — the host-and-device header of the EDI receiving stage (csrc/edirx_plan.hpp) under ASan + UBSan, as a stand-alone program.
// Its inputs are lists the model wrote (u32 count, then per item u32 length and the bytes, little-endian); every item is copied to a heap
// buffer of exactly its size before the header sees it, so a read past a truncated or lying length field is caught.
//   check packets.bin                      edirx_check_packet of every item -> its kind (0 bad, 1 AF, 2 PF, 3 PF with FEC) and m_max
//   walk afs.bin out.eti                   edirx_walk of every item (an AF packet whose CRC is not looked at) -> 0 or why refused; the
//                                          frames of the accepted ones by edirx_rebuild
//   stream packets.bin depth cuts out.eti  one stream through edirx_window_step, with a flush at the end and (cuts = 1) the kernels' per-push
//                                          bookkeeping reset after every packet; the groups' bytes placed by edirx_place, the AF packets of
//                                          the ready groups checked, walked and rebuilt.  Groups with erasures are counted, not decoded (the
//                                          decoder is a kernel).  Prints the 15 counters.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dabtools_amd/csrc/edirx_plan.hpp"

using namespace dabhip;

namespace {
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Item {
  uint8_t* p;
  int64_t n;
};

std::vector<Item> read_items(const char* path)
{
  FILE* fp = std::fopen(path, "rb");
  CHECK(fp != nullptr);
  uint32_t count = 0;
  CHECK(std::fread(&count, 4, 1, fp) == 1);
  std::vector<Item> out;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t n = 0;
    CHECK(std::fread(&n, 4, 1, fp) == 1);
    Item it = {new uint8_t[n], n};                       // exactly its size (new uint8_t[0] is a valid, unreadable place)
    CHECK(n == 0 || std::fread(it.p, 1, n, fp) == n);
    out.push_back(it);
  }
  std::fclose(fp);
  return out;
}

void free_items(std::vector<Item>& v)
{
  for (Item& it : v) delete[] it.p;
}

struct Left {
  EdirxGroup g;
  uint8_t* bytes;
  bool ready;
};

struct HostSink {
  uint8_t* buf[kEdirxMaxDepth] = {};
  uint8_t* cur = nullptr;
  std::vector<Left> left;
  void joined(EdirxStream& st, int e)
  {
    if (st.open[e].nrecv == 1) {
      CHECK(buf[e] == nullptr);
      buf[e] = new uint8_t[kEdirxStride]();
    }
    cur = buf[e];
  }
  void finalise(EdirxStream& st, int e, bool ready)
  {
    left.push_back(Left{st.open[e], buf[e], ready});
    buf[e] = nullptr;
  }
};

// what the frame kernel does with a ready group; returns 0 frame, 1 needs the decoder, 2 crc, 3 refused
int group_to_frame(const Left& x, uint8_t* frame, EdirxLayout& lay)
{
  const EdirxGroup& g = x.g;
  if (g.kind == kEdirxPfFec && g.nrecv < g.fcount) {
    const int c = g.fcount * g.plen / (g.rsk + kEdiRsP);
    for (int w = 0; w < c; ++w) {
      uint8_t pos[256];
      const int n = edirx_word_erasures(g.mask, g.fcount, g.rsk, w, pos);
      CHECK(n <= kEdiRsP);
      for (int i = 1; i < n; ++i) CHECK(pos[i] > pos[i - 1]);
    }
    return 1;
  }
  const int len = edirx_af_bytes(g);
  CHECK(len >= 1 && len <= kEdirxMaxPayload);
  uint8_t* pk = new uint8_t[len];
  const int body = (g.fcount - 1) * g.plen;
  for (int i = 0; i < len; ++i) {
    int at = i;
    if (g.kind == kEdirxPfFec) at = i / g.rsk * (g.rsk + kEdiRsP) + i % g.rsk;
    else if (g.kind == kEdirxPf && g.fcount > 1 && i >= body) at = kEdirxTail + i - body;
    CHECK(at < kEdirxStride);
    pk[i] = x.bytes[at];
  }
  int verdict = 0;
  const bool good = len >= kEdiAfOver && pk[0] == 'A' && pk[1] == 'F' && static_cast<int64_t>(edirx_get32(pk + 2)) + kEdiAfOver == len && (pk[8] & 0xF0) == 0x90 &&
                    pk[9] == 'T' && edi_crc16(pk, len - 2) == edirx_get16(pk + len - 2);
  if (!good) verdict = 2;
  else if (edirx_walk(pk, len, lay)) verdict = 3;
  else edirx_rebuild(pk, lay, frame);
  delete[] pk;
  return verdict;
}

int run_stream(const char* in, int depth, int cuts, const char* outpath)
{
  std::vector<Item> items = read_items(in);
  FILE* out = std::fopen(outpath, "wb");
  CHECK(out != nullptr && depth >= 1 && depth <= kEdirxMaxDepth);
  EdirxStream* st = new EdirxStream();
  int64_t cnt[kEdirxCntN] = {0};
  long needs_rs = 0;
  HostSink sink;
  uint8_t* frame = new uint8_t[kEdiEti];
  const auto drain = [&]() {
    for (Left& x : sink.left) {
      if (x.ready) {
        EdirxLayout lay = {};
        const int v = group_to_frame(x, frame, lay);
        if (v == 1) ++needs_rs;
        else if (v == 2) ++cnt[kEdirxCntCrcFailed];
        else if (v == 3) ++cnt[kEdirxCntRefused];
        else {
          CHECK(std::fwrite(frame, 1, kEdiEti, out) == static_cast<size_t>(kEdiEti));
          cnt[kEdirxCntItemsIgnored] += lay.items_ignored;
          cnt[kEdirxCntWithAtst] += lay.atstf;
          ++cnt[kEdirxCntFrames];
        }
      }
      delete[] x.bytes;
    }
    sink.left.clear();
  };
  for (const Item& it : items) {
    if (cuts)
      for (int e = 0; e < depth; ++e) { st->open[e].local = -1; st->open[e].carried = st->open[e].used; }
    const EdirxHdr h = edirx_check_packet(it.p, it.n);
    sink.cur = nullptr;
    const int e = edirx_window_step(*st, depth, h, cnt, sink);
    if (e >= 0) {
      CHECK(sink.cur != nullptr);
      int at, step;
      edirx_place(h, &at, &step);
      CHECK(at + (h.plen - 1) * step < kEdirxStride && h.head + h.plen == it.n);
      for (int j = 0; j < h.plen; ++j) sink.cur[at + j * step] = it.p[h.head + j];
    }
    int open = 0;
    for (int i = 0; i < depth; ++i)
      if (st->open[i].used) {
        ++open;
        CHECK(((st->open[i].seq - st->next) & 0xFFFF) < depth);
      }
    CHECK(open <= depth);
    drain();
  }
  edirx_flush(*st, depth, cnt, sink);
  drain();
  for (int e = 0; e < kEdirxMaxDepth; ++e) CHECK(sink.buf[e] == nullptr && !st->open[e].used);
  std::fclose(out);
  std::printf("ok edirx-units\ncounters:");
  for (int i = 0; i < kEdirxCntN; ++i) std::printf(" %lld", static_cast<long long>(cnt[i]));
  std::printf(" needs_rs %ld\n", needs_rs);
  delete[] frame;
  delete st;
  free_items(items);
  return 0;
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "check")) {
    std::vector<Item> items = read_items(argv[2]);
    std::printf("ok edirx-units\nkinds:");
    for (const Item& it : items) {
      const EdirxHdr h = edirx_check_packet(it.p, it.n);
      std::printf(" %d:%d", h.kind, h.kind == kEdirxPfFec ? edirx_m_max(h.rsk, h.fcount) : 0);
    }
    std::printf("\n");
    free_items(items);
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "walk")) {
    std::vector<Item> items = read_items(argv[2]);
    FILE* out = std::fopen(argv[3], "wb");
    CHECK(out != nullptr);
    uint8_t* frame = new uint8_t[kEdiEti];
    std::printf("ok edirx-units\nverdicts:");
    for (const Item& it : items) {
      CHECK(it.n >= kEdiAfOver && it.n <= kEdirxMaxPayload);
      EdirxLayout* lay = new EdirxLayout();
      const int v = edirx_walk(it.p, static_cast<int>(it.n), *lay);
      std::printf(" %d", v);
      if (v == 0) {
        edirx_rebuild(it.p, *lay, frame);
        CHECK(std::fwrite(frame, 1, kEdiEti, out) == static_cast<size_t>(kEdiEti));
      }
      delete lay;
    }
    std::printf("\n");
    delete[] frame;
    std::fclose(out);
    free_items(items);
    return 0;
  }
  if (argc == 6 && !std::strcmp(argv[1], "stream")) return run_stream(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), argv[5]);
  std::printf("usage: edirx_units check packets.bin | walk afs.bin out.eti | stream packets.bin depth cuts out.eti\n");
  return 1;
}
