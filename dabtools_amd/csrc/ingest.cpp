// ingest.cpp — the ingest stage's host object (include/dabhip.h: dabhip_ingest): per stream the positions and the carried samples, per push the
// plan (ingest_plan.hpp), the uploads, the energy reduction of the streams whose gain window closes, and one launch of k_ingest.hip's kernel
// for all streams.  The tuned mode (dabhip_ingest_create_tuned) has nchannels output streams per input stream: one descriptor per output stream,
// the channels of a stream sharing its plan, carry and input, and the keep kernel's descriptors (one per input stream) behind them.  Every push
// ends in a stream synchronise (hip_util.hpp: what the runtime keeps of a stream that nobody synchronises).
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "ingest.hpp"
#include "ingest_plan.hpp"
#include "stage_frame.hpp"

using namespace dabhip;

namespace {
const char* const kStages[4] = {"upload", "energy", "resample", "keep"};
}

struct dabhip_ingest {
  int nstreams = 0, format = 0, sample_bytes = 0;
  int nchannels = 1, nouts = 0;                  // output streams: nstreams * nchannels, stream-major
  bool tuned = false;
  std::vector<uint32_t> step;                    // tuned: the NCO step per channel
  IngestRatio ratio;
  bool auto_gain = false;
  std::vector<IngestStreamState> st;
  std::vector<uint32_t> gain;                    // per output stream; 0 while its window is open
  DeviceBuffer<uint32_t> table, nco;
  DeviceBuffer<uint8_t> carry[2], stage, out;
  DeviceBuffer<IngestDesc> descs;
  DeviceBuffer<unsigned long long> energy;
  size_t carry_stride = 0;
  int cur = 0;                                   // carry[cur] holds what the last push kept
  std::vector<size_t> out_off, out_bytes;
  StageFrame<4> f{"ingest", kStages};
};

namespace {
// the push proper: nsamples[b] samples of stream b at src[b] (device memory, aligned to a sample).  Returns the output bytes, < 0 on error.
int64_t push_device(dabhip_ingest* d, const std::vector<const void*>& src, const std::vector<int64_t>& nsamples, bool uploaded)
{
  const int ns = d->nstreams, nc = d->nchannels, no = d->nouts;
  std::vector<IngestStreamState> next = d->st;
  std::vector<IngestPush> plan(static_cast<size_t>(ns));
  std::vector<IngestDesc> h(static_cast<size_t>(d->tuned ? no + ns : no));       // tuned: the keep kernel's, one per input stream, at the end
  size_t out_total = 0;
  int64_t max_nout = 0, max_keep = 0;
  bool closing = false;
  for (int b = 0; b < ns; ++b) {
    IngestStreamState& s = next[static_cast<size_t>(b)];
    const IngestPush p = plan[static_cast<size_t>(b)] = d->tuned ? ingest_tune_plan_push(d->ratio, s, nsamples[static_cast<size_t>(b)]) : ingest_plan_push(d->ratio, s, nsamples[static_cast<size_t>(b)]);
    if (p.nout > (int64_t(1) << 30)) { set_error("ingest_push: more than 2^30 output samples of one stream in one push"); return -1; }
    if (static_cast<size_t>(p.keep) * d->sample_bytes > d->carry_stride) { set_error("ingest_push: internal: the carry outgrew its buffer"); return -1; }
    for (int c = 0; c < nc; ++c) {
      d->out_off[static_cast<size_t>(b * nc + c)] = out_total;
      out_total += round_up(static_cast<size_t>(p.nout) * 2, 256);
    }
    max_nout = std::max(max_nout, p.nout);
    max_keep = std::max(max_keep, p.keep);
    closing = closing || p.closes;
  }
  if (!d->out.reserve(out_total ? out_total : 1) || !d->descs.reserve(h.size()) || !d->energy.reserve(static_cast<size_t>(no))) return -1;
  for (int o = 0; o < no; ++o) {
    const int b = o / nc;
    const IngestPush& p = plan[static_cast<size_t>(b)];
    IngestDesc& x = h[static_cast<size_t>(o)];
    x.carry = d->carry[d->cur].get() + static_cast<size_t>(b) * d->carry_stride;
    x.keep = d->carry[d->cur ^ 1].get() + static_cast<size_t>(b) * d->carry_stride;
    x.src = src[static_cast<size_t>(b)];
    x.out = d->out.get() + d->out_off[static_cast<size_t>(o)];
    x.carry_from = p.carry_from;
    x.new_from = p.new_from;
    x.end = p.end;
    x.first_out = p.first_out;
    x.keep_from = p.keep_from;
    x.nout = static_cast<int32_t>(p.nout);
    x.gain = d->gain[static_cast<size_t>(o)];
    x.energy_slot = p.closes ? o : -1;
    x.step = d->tuned ? d->step[static_cast<size_t>(o % nc)] : 0;
  }
  for (int b = 0; b < ns && d->tuned; ++b) h[static_cast<size_t>(no + b)] = h[static_cast<size_t>(b * nc)];
  const IngestDesc* keep_descs = d->descs.get() + (d->tuned ? no : 0);
  StageFrame<4>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  hipStream_t st = f.stream;
  std::vector<uint32_t> gain = d->gain;
  if (!uploaded && !f.mark(0)) return -1;
  if (!f.mark(1)) return -1;
  if (closing) {
    std::vector<unsigned long long> e(static_cast<size_t>(no), 0);
    if (!ok(hipMemcpyAsync(d->descs.get(), h.data(), h.size() * sizeof(IngestDesc), hipMemcpyHostToDevice, st), "descriptors")) return -1;
    if (d->tuned) {                                // the energy of OUTPUTS [0, W) of every channel: the tuned kernel's energy form adds to zeroed slots
      if (!ok(hipMemsetAsync(d->energy.get(), 0, e.size() * sizeof(unsigned long long), st), "energy") ||
          !ok(launch_ingest_tune(d->format, d->descs.get(), no, 0, d->table.get(), d->nco.get(), d->energy.get(), d->ratio.L, d->ratio.M, d->ratio.T, st), "energy launch"))
        return -1;
    } else if (!ok(launch_ingest_energy(d->format, d->descs.get(), ns, d->energy.get(), st), "energy launch")) {
      return -1;
    }
    if (!ok(hipMemcpyAsync(e.data(), d->energy.get(), e.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "energy") || !ok(hipStreamSynchronize(st), "energy")) return -1;
    for (int o = 0; o < no; ++o)
      if (plan[static_cast<size_t>(o / nc)].closes) h[static_cast<size_t>(o)].gain = gain[static_cast<size_t>(o)] = ingest_auto_gain(e[static_cast<size_t>(o)]);
  }
  if (!f.mark(2) || !ok(hipMemcpyAsync(d->descs.get(), h.data(), h.size() * sizeof(IngestDesc), hipMemcpyHostToDevice, st), "descriptors") ||
      !ok(d->tuned ? launch_ingest_tune(d->format, d->descs.get(), no, static_cast<int>(max_nout), d->table.get(), d->nco.get(), nullptr, d->ratio.L, d->ratio.M, d->ratio.T, st)
                   : launch_ingest_resample(d->format, d->descs.get(), ns, static_cast<int>(max_nout), d->table.get(), d->ratio.L, d->ratio.M, d->ratio.T, st),
          "resample launch") ||
      !f.mark(3) || !ok(launch_ingest_keep(d->format, keep_descs, ns, max_keep, st), "keep launch") || !f.mark(4) || !f.finish())
    return -1;
  d->st = next;
  d->gain = gain;
  d->cur ^= 1;
  int64_t total = 0;
  for (int o = 0; o < no; ++o) total += static_cast<int64_t>(d->out_bytes[static_cast<size_t>(o)] = static_cast<size_t>(plan[static_cast<size_t>(o / nc)].nout) * 2);
  return total;
}
}  // namespace

namespace {
// the table as the kernels hold it: reversed, in pairs, rows padded by a word (ingest.hpp)
std::vector<uint32_t> table_words(const IngestRatio& r, const std::vector<int16_t>& taps)
{
  std::vector<uint32_t> words(r.lds_table_bytes() / 4 + 2, 0);
  for (int p = 0; p < r.L && !r.bypass(); ++p)
    for (int j = 0; j < r.T / 2; ++j) {
      const uint16_t lo = static_cast<uint16_t>(taps[static_cast<size_t>(p) * r.T + (r.T - 1 - 2 * j)]), hi = static_cast<uint16_t>(taps[static_cast<size_t>(p) * r.T + (r.T - 2 - 2 * j)]);
      words[static_cast<size_t>(p) * r.lds_row_words() + j] = lo | static_cast<uint32_t>(hi) << 16;
    }
  return words;
}
// the object behind both creators, once everything that can be refused has been: step empty = the plain mode, one channel
dabhip_ingest* make(const char* who, int device, int nstreams, int format, const IngestRatio& r, uint32_t gain, const std::vector<uint32_t>& words, const std::vector<uint32_t>& step)
{
  dabhip_ingest* d = new (std::nothrow) dabhip_ingest;
  if (!d) return nullptr;
  StageFrame<4>& f = d->f;
  d->nstreams = nstreams;
  d->tuned = !step.empty();
  d->nchannels = d->tuned ? static_cast<int>(step.size()) : 1;
  d->nouts = nstreams * d->nchannels;
  d->step = step;
  d->format = format;
  d->sample_bytes = ingest_sample_bytes(format);
  d->ratio = r;
  d->auto_gain = gain == 0;
  d->st.assign(static_cast<size_t>(nstreams), IngestStreamState{});
  for (auto& s : d->st) s.window_open = d->auto_gain;
  d->gain.assign(static_cast<size_t>(d->nouts), gain);
  d->out_off.assign(static_cast<size_t>(d->nouts), 0);
  d->out_bytes.assign(static_cast<size_t>(d->nouts), 0);
  // while the window is open everything is carried: fewer than W samples, tuned fewer than complete output W - 1
  const int64_t held = d->tuned ? ingest_samples_for_outputs(r, kIngestGainWindow) : kIngestGainWindow;
  d->carry_stride = round_up(static_cast<size_t>(d->auto_gain ? held : std::max(r.T, 1)) * d->sample_bytes, 16);
  bool good = f.open(device, std::string(who) + ": no HIP device") && d->table.reserve(words.size()) && d->carry[0].reserve(d->carry_stride * nstreams) &&
              d->carry[1].reserve(d->carry_stride * nstreams) &&
              f.ok(hipMemcpyAsync(d->table.get(), words.data(), words.size() * 4, hipMemcpyHostToDevice, f.stream), "table upload");
  const std::vector<uint32_t> nco = d->tuned ? ingest_tune_nco_words() : std::vector<uint32_t>();
  if (good && d->tuned) good = d->nco.reserve(nco.size()) && f.ok(hipMemcpyAsync(d->nco.get(), nco.data(), nco.size() * 4, hipMemcpyHostToDevice, f.stream), "NCO table upload");
  good = good && f.ok(hipStreamSynchronize(f.stream), "table upload");
  if (!good) { delete d; return nullptr; }
  return d;
}
}  // namespace

extern "C" dabhip_ingest* dabhip_ingest_create(int device, int nstreams, int format, int64_t rate_hz, uint32_t gain)
{
  if (nstreams <= 0 || nstreams > 65535) { set_error("ingest_create: nstreams must be 1 .. 65535"); return nullptr; }
  if (format < 0 || format >= kIngestFormats) { set_error("ingest_create: unknown format " + std::to_string(format) + " (0 = cu8, 1 = cs8, 2 = cs16, 3 = cf32)"); return nullptr; }
  if (gain > kIngestMaxGain) { set_error("ingest_create: gain must be below 2^24 (0 = automatic)"); return nullptr; }
  IngestRatio r;
  const std::string why = ingest_ratio(rate_hz, &r);
  if (!why.empty()) { set_error("ingest_create: " + why); return nullptr; }
  std::vector<int16_t> taps;
  if (!r.bypass()) {
    taps = ingest_design_taps(r, rate_hz);
    const std::string bad = ingest_check_taps(r, taps.data());
    if (!bad.empty()) { set_error("ingest_create: " + bad); return nullptr; }
  }
  return make("ingest_create", device, nstreams, format, r, gain, table_words(r, taps), {});
}

extern "C" dabhip_ingest* dabhip_ingest_create_tuned(int device, int nstreams, int format, int64_t rate_hz, uint32_t gain, const int64_t* offsets_hz, int nchannels)
{
  if (format < 0 || format >= kIngestFormats) { set_error("ingest_create_tuned: unknown format " + std::to_string(format) + " (0 = cu8, 1 = cs8, 2 = cs16, 3 = cf32)"); return nullptr; }
  if (gain > kIngestMaxGain) { set_error("ingest_create_tuned: gain must be below 2^24 (0 = automatic)"); return nullptr; }
  IngestRatio r;
  const std::string why = ingest_tune_check(nstreams, rate_hz, offsets_hz, nchannels, &r);
  if (!why.empty()) { set_error("ingest_create_tuned: " + why); return nullptr; }
  std::vector<int16_t> taps;
  if (!r.bypass()) {
    taps = ingest_tune_design_taps(r, rate_hz);
    const std::string bad = ingest_check_taps(r, taps.data());
    if (!bad.empty()) { set_error("ingest_create_tuned: " + bad); return nullptr; }
  }
  std::vector<uint32_t> step;
  for (int c = 0; c < nchannels; ++c) step.push_back(ingest_tune_step(rate_hz, offsets_hz[c]));
  return make("ingest_create_tuned", device, nstreams, format, r, gain, table_words(r, taps), step);
}

extern "C" void dabhip_ingest_destroy(dabhip_ingest* d) { delete d; }

extern "C" int64_t dabhip_ingest_push(dabhip_ingest* d, const void* const* src, const size_t* nbytes, int on_device)
{
  if (!d || !src || !nbytes) { set_error("ingest_push: null argument"); return -1; }
  const SamplePush p = plan_sample_push("ingest_push", static_cast<size_t>(d->sample_bytes), src, nbytes, on_device != 0, d->nstreams, [](int, int64_t n) { return n; });
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  std::vector<const void*> dev(src, src + d->nstreams);
  if (!d->f.use_device() || (!on_device && !d->f.upload(d->stage, p, src, dev))) return -1;
  return push_device(d, dev, p.nsamples, !on_device);
}

extern "C" int dabhip_ingest_skip(dabhip_ingest* d, int64_t n)
{
  if (!d || n < 0) { set_error("ingest_skip: bad argument"); return -1; }
  if (d->auto_gain) { set_error("ingest_skip: only with an explicit gain"); return -1; }
  const int64_t through = ingest_skip_through(d->ratio, n);
  if (through) {                                   // samples of value 0 in the 16-bit domain: cu8's byte 127, zero bytes otherwise
    const std::vector<uint8_t> zeros(static_cast<size_t>(through) * d->sample_bytes, d->format == 0 ? 127 : 0);
    std::vector<const void*> src(static_cast<size_t>(d->nstreams), zeros.data());
    const std::vector<size_t> nbytes(static_cast<size_t>(d->nstreams), zeros.size());
    if (dabhip_ingest_push(d, src.data(), nbytes.data(), 0) < 0) return -1;
  }
  for (auto& s : d->st) ingest_skip_rest(d->ratio, s, n - through);
  std::fill(d->out_bytes.begin(), d->out_bytes.end(), size_t(0));
  return 0;
}

extern "C" int dabhip_ingest_output(const dabhip_ingest* d, int stream, const uint8_t** dev, size_t* nbytes)
{
  if (!d || stream < 0 || stream >= d->nouts || !dev || !nbytes) { set_error("ingest_output: bad argument"); return -1; }
  *dev = d->out.get() + d->out_off[static_cast<size_t>(stream)];
  *nbytes = d->out_bytes[static_cast<size_t>(stream)];
  return 0;
}

extern "C" int64_t dabhip_ingest_read(const dabhip_ingest* d, int stream, uint8_t* dst, size_t cap)
{
  if (!d || stream < 0 || stream >= d->nouts || (!dst && cap)) { set_error("ingest_read: bad argument"); return -1; }
  const size_t n = d->out_bytes[static_cast<size_t>(stream)];
  if (n > cap) { set_error("ingest_read: buffer too small"); return -1; }
  if (!d->f.use_device()) return -1;
  if (n && !d->f.ok(blocking_copy(dst, d->out.get() + d->out_off[static_cast<size_t>(stream)], n, hipMemcpyDeviceToHost), "read")) return -1;
  return static_cast<int64_t>(n);
}

extern "C" uint32_t dabhip_ingest_gain(const dabhip_ingest* d, int stream)
{
  return d && stream >= 0 && stream < d->nouts ? d->gain[static_cast<size_t>(stream)] : 0;
}

extern "C" int dabhip_ingest_stage_ms(const dabhip_ingest* d, const char** names, float* ms, int cap)
{
  if (!d || !names || !ms) { set_error("ingest_stage_ms: null argument"); return -1; }
  return d->f.stage_ms(names, ms, cap);
}
