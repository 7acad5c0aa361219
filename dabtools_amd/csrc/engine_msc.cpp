// engine_msc.cpp — TF slots, FIC decode and MSC decode (see engine.hpp for the pipeline).
#include "engine_detail.hpp"

namespace dabhip {

namespace {
void unpack_bits(const uint32_t* words, int nbits, uint8_t* bytes)
{
  for (int i = 0; i < nbits; ++i) bytes[i] = static_cast<uint8_t>((words[i >> 5] >> (i & 31)) & 1u);
}
}  // namespace

bool Engine::upload_small(const SmallUpload* items, int n, hipStream_t s, SmallStage& stage)
{
  PinnedBuffer<uint32_t>& staging = stage.words;
  size_t total = 0;
  bool words = true;
  for (int i = 0; i < n; ++i) {
    total += items[i].bytes;
    words = words && items[i].bytes % 4 == 0 && reinterpret_cast<uintptr_t>(items[i].src) % 4 == 0;
  }
  if (!words || total > kSmallUploadBytes) {
    for (int i = 0; i < n; ++i)
      if (items[i].bytes && !check(hipMemcpyAsync(items[i].dst, items[i].src, items[i].bytes, hipMemcpyHostToDevice, s), "work list upload")) return false;
    return true;
  }
  if (staging.size() < kSmallUploadBytes / 4 && !staging.resize(kSmallUploadBytes / 4)) return false;   // once: the buffer never moves while a kernel may read it
  // the stage's previous launch reads these words when it runs: still in flight -> wait for it (see engine.hpp; not reached by today's callers)
  if (stage.armed && hipEventQuery(stage.done) == hipErrorNotReady && !check(hipEventSynchronize(stage.done), "work list staging")) return false;
  (void)hipGetLastError();
  if (!stage.done && !check(stage.done.create(false), "hipEventCreate")) return false;
  size_t at = 0;
  HostWordsArgs hw{};
  int k = 0;
  for (int i = 0; i < n; ++i) {
    if (items[i].bytes == 0) continue;
    const uint32_t* src = static_cast<const uint32_t*>(items[i].src);
    if (!items[i].pinned) {
      std::memcpy(staging.data() + at, items[i].src, items[i].bytes);
      src = staging.data() + at;
      at += items[i].bytes / 4;
    }
    hw.set(k, src, items[i].dst, items[i].bytes / 4);
    if (++k == 4) {
      if (!check(launch_host_words(hw, s), "work list upload")) return false;
      hw = HostWordsArgs{};
      k = 0;
    }
  }
  if (k != 0 && !check(launch_host_words(hw, s), "work list upload")) return false;
  stage.armed = check(hipEventRecord(stage.done, s), "work list staging event");
  return stage.armed;
}

// regroup + Viterbi over an uploaded batch: queued only; ev_msc_[0..2] bracket the two stages
bool Engine::launch_decode_batch(const DecodeBatch& b, const uint32_t* bits, const int* d_stream_cif_base, const uint32_t* prbs, uint8_t* out,
                                 int record_stride)
{
  if (b.groups.empty()) {                                 // nothing to decode: the three stamps still exist for msc_collect
    return record(ev_msc_[0], stream_) && record(ev_msc_[1], stream_) && record(ev_msc_[2], stream_);
  }
  const int* ids = d_job_ids_.get();
  const int row_words = kCifWords * (soft_bits_ ? 4 : 1);
  const int ntiles = static_cast<int>(b.job_ids.size() / 64);
  if (!record(ev_msc_[0], stream_)) return false;
  if (!check(launch_regroup(soft_bits_, ids, ntiles, d_jobs_.get(), d_stream_cif_base, bits, d_grouped_.get(), stream_, limits_.regroup_tiles, &report_.regroup), "regroup launch")) return false;
  if (!record(ev_msc_[1], stream_)) return false;
  // the form the knobs' rule or set_decoder_forms picks (decoder_form.hpp), slice by slice (a small batch -- one wave per code word, all lengths longest
  // first, its decisions in the survivor-record buffer -- is one slice: worklist.hpp)
  const int form = msc_form(knobs_, msc_form_, soft_bits_ != 0, b.wave_form, static_cast<int>(b.groups.size()));
  msc_ran_ |= 1u << form;
  report_.decoder_planned = static_cast<int64_t>(b.slice_start.size()) - 1;
  for (size_t sl = 0; sl + 1 < b.slice_start.size(); ++sl) {
    const int g0 = b.slice_start[sl];
    const ViterbiLaunch v{d_groups_.get() + g0, b.slice_start[sl + 1] - g0, ids, d_plans_.get(), d_grouped_.get(), row_words, d_decisions_.get(), prbs, out, record_stride};
    if (!check(launch_viterbi_form(form, soft_bits_, v, stream_), "viterbi launch")) return false;
    ++report_.decoder;
  }
  if (!record(ev_msc_[2], stream_)) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------
bool Engine::reserve_tf_slots(int nslots, int msc_rows)
{
  if (msc_rows < 0) msc_rows = 4 * nslots + kRowLead + 1;
  // growth discards contents: callers reserve before filling
  const size_t bits = soft_bits_ ? 4 : 1;
  if (nslots > tf_slots_) {
    if (!d_fic_bits_.reserve(static_cast<size_t>(nslots) * kFicWords * bits) || !d_fibs_.reserve(static_cast<size_t>(nslots) * 384) ||
        !d_fib_ok_.reserve(static_cast<size_t>(nslots) * 12))
      return false;
    tf_slots_ = nslots;
  }
  if (msc_rows > msc_rows_) {
    if (!d_msc_bits_.reserve(static_cast<size_t>(msc_rows) * kCifWords * bits)) return false;
    msc_rows_ = msc_rows;
  }
  return true;
}

// S3: host 0/1 bytes of one TF -> FIC row of `slot`, MSC scattered into the planar logical rows (single stream,
// CIF 0 at row kRowLead), the same layout demap_kernel<true> produces.  With soft decisions on the bytes are signed 4-bit
// values (-7 .. 7 as int8; > 0: bit 0) and the rows hold a nibble per value: word u / 8 of a plane, nibble u % 8.
bool Engine::store_tf_bytes(int slot, const uint8_t* fic_bytes, const uint8_t* msc_bytes)
{
  const int bits = soft_bits_ ? 4 : 1, per = 32 / bits;
  const uint32_t vmask = soft_bits_ ? 15u : 1u;
  const size_t fic_words = static_cast<size_t>(kFicWords) * bits, row_words = static_cast<size_t>(kCifWords) * bits, plane_words = 108u * bits;
  std::vector<uint32_t> f(fic_words, 0u), plane(plane_words);
  for (int i = 0; i < kFicBits; ++i) f[i / per] |= (static_cast<uint32_t>(fic_bytes[i]) & vmask) << (bits * (i % per));
  if (!check(blocking_copy(d_fic_bits_.get() + static_cast<size_t>(slot) * fic_words, f.data(), f.size() * 4, hipMemcpyHostToDevice), "fic upload")) return false;
  for (int q = 0; q < 4; ++q) {
    const uint8_t* cif = msc_bytes + static_cast<size_t>(q) * kCifBits;
    for (int r = 0; r < 16; ++r) {
      std::fill(plane.begin(), plane.end(), 0u);
      for (int u = 0; u < kCifBits / 16; ++u) plane[u / per] |= (static_cast<uint32_t>(cif[16 * u + r]) & vmask) << (bits * (u % per));
      const size_t row = static_cast<size_t>(kRowLead + 4 * slot + q - kPlaneRowsBack[r]);
      // plane r occupies words [108 r, 108 r + 108) (x 4 with soft values) of the logical row (layout of demap_kernel<true>)
      if (!check(blocking_copy(d_msc_bits_.get() + row * row_words + r * plane_words, plane.data(), plane_words * 4, hipMemcpyHostToDevice), "msc upload")) return false;
    }
  }
  return true;
}

bool Engine::recycle_tf_slots(int used_slots, int keep_slots)
{
  // FIC rows / FIB records: the newest keep_slots; logical CIF rows: everything from 15 rows before the oldest kept CIF
  const size_t bits = soft_bits_ ? 4 : 1;
  const int src_slot = used_slots - keep_slots;
  const size_t row_src = static_cast<size_t>(4 * src_slot), nrows = static_cast<size_t>(4 * keep_slots + kRowLead);
  if (!d_bytes_.reserve(std::max(nrows * kCifWords * 4 * bits, static_cast<size_t>(keep_slots) * kFicWords * 4 * bits))) return false;
  auto mv = [&](void* base, size_t unit, size_t src, size_t n) {
    uint8_t* b = static_cast<uint8_t*>(base);
    return check(blocking_copy(d_bytes_.get(), b + src * unit, n * unit, hipMemcpyDeviceToDevice), "slot move") &&
           check(blocking_copy(b, d_bytes_.get(), n * unit, hipMemcpyDeviceToDevice), "slot move");
  };
  return mv(d_fic_bits_.get(), kFicWords * 4 * bits, src_slot, keep_slots) && mv(d_fibs_.get(), 384, src_slot, keep_slots) &&
         mv(d_fib_ok_.get(), 12, src_slot, keep_slots) && mv(d_msc_bits_.get(), kCifWords * 4 * bits, row_src, nrows);
}

// What the OFDM stage of the LAST decode() / feed() left for transmission frame `tf` (0-based among the stream's TF slots of that
// decode, carried slots of a session first) of `stream`: the content of tf->fic_symbols_demapped / msc_symbols_demapped (dab.h:27-33)
// as the batch path holds it -- FIC row in natural order, MSC values gathered back out of the planar logical rows the demapper
// scattered them into.  Hard decisions: 0 / 1; soft decisions: the signed 4-bit values.  A TF whose MSC part the decode deferred (lock-in skip) is
// completed first, together with all other deferred TFs of that decode.
bool Engine::read_demapped_tf(int stream, int tf, int8_t* fic_out, int8_t* msc_out)
{
  if (stream < 0 || stream >= nstreams_ || static_cast<int>(carry_.size()) <= stream || tf < 0 || tf >= carry_[stream].prev_used) {
    set_error("demapped_tf: no such stream / transmission frame in the last decode");
    return false;
  }
  if (!check(hipSetDevice(device_), "hipSetDevice")) return false;
  // lock-in skip: the MSC part of this TF was deferred -- complete the last decode's deferred frames first (once; all of them)
  const StreamCarry& sc = carry_[stream];
  if (static_cast<size_t>(tf) < sc.msc_missing.size() && sc.msc_missing[tf]) {
    if (!last_.pending || tf < sc.last_keep) {
      set_error("demapped_tf: the MSC symbols of this transmission frame were not demodulated (it could not be locked) and its samples belong to an earlier segment");
      return false;
    }
    if (!complete_deferred()) return false;
  }
  const int bits = soft_bits_ ? 4 : 1, per = 32 / bits;
  const size_t fic_words = static_cast<size_t>(kFicWords) * bits, row_words = static_cast<size_t>(kCifWords) * bits, plane_words = 108u * bits;
  std::vector<uint32_t> f(fic_words), rows(static_cast<size_t>(kRowLead + 4) * row_words);
  const size_t slot = static_cast<size_t>(sc.prev_tf_base) + tf, row0 = static_cast<size_t>(sc.prev_row_base) + 4 * tf - kRowLead;
  if (!check(blocking_copy(f.data(), d_fic_bits_.get() + slot * fic_words, f.size() * 4, hipMemcpyDeviceToHost), "fic download") ||
      !check(blocking_copy(rows.data(), d_msc_bits_.get() + row0 * row_words, rows.size() * 4, hipMemcpyDeviceToHost), "msc download"))
    return false;
  auto value = [&](uint32_t w, int k) -> int8_t {
    const uint32_t v = (w >> (bits * k)) & (soft_bits_ ? 15u : 1u);
    return static_cast<int8_t>(soft_bits_ ? static_cast<int>(v ^ 8u) - 8 : static_cast<int>(v));
  };
  for (int i = 0; i < kFicBits; ++i) fic_out[i] = value(f[i / per], i % per);
  for (int q = 0; q < 4; ++q)
    for (int i = 0; i < kCifBits; ++i) {
      const int r = i & 15, u = i >> 4;
      const size_t row = static_cast<size_t>(kRowLead + q - kPlaneRowsBack[r]);       // transmitted CIF q of this TF
      msc_out[static_cast<size_t>(q) * kCifBits + i] = value(rows[row * row_words + r * plane_words + u / per], u % per);
    }
  return true;
}

// S2 / stage_demap: the TF was demapped in NATURAL order (demap_kernel<false>) into FIC slot `slot`, CIF rows 4*slot..
bool Engine::unpack_tf_slot(int slot, uint8_t* fic_bytes, uint8_t* msc_bytes)
{
  if (!hard_only("unpack_tf_slot")) return false;
  std::vector<uint32_t> f(kFicWords), m(kMscWords);
  if (!check(blocking_copy(f.data(), d_fic_bits_.get() + static_cast<size_t>(slot) * kFicWords, f.size() * 4, hipMemcpyDeviceToHost), "fic download") ||
      !check(blocking_copy(m.data(), d_msc_bits_.get() + static_cast<size_t>(slot) * kMscWords, m.size() * 4, hipMemcpyDeviceToHost), "msc download"))
    return false;
  unpack_bits(f.data(), kFicBits, fic_bytes);
  unpack_bits(m.data(), kMscBits, msc_bytes);
  return true;
}

bool Engine::fic_decode_slots(int first, int n, uint8_t* fibs_host, uint8_t* ok_host)
{
  return fic_decode_slots_async(first, n, fibs_host, ok_host, stream_) && check(hipStreamSynchronize(stream_), "fic decode");
}

// the same without waiting: kernels on the main stream, the FIB / flag download on `copy` (ordered after them by an event)
bool Engine::fic_decode_slots_async(int first, int n, uint8_t* fibs_host, uint8_t* ok_host, hipStream_t copy)
{
  if (n <= 0) return true;
  const int bits = soft_bits_ ? 4 : 1;
  const int pid = plan_table_.id(make_codeword_plan(fic_plan(), 0, 0));
  // record i of this call = FIC block 4 * first + i; 64 blocks per wave, interleaved word by word by fic_group_kernel
  const int nblocks = 4 * n, ntiles = (nblocks + 63) / 64, block_words = 72 * bits;
  std::vector<int> ids(static_cast<size_t>(ntiles) * 64, -1);
  for (int i = 0; i < nblocks; ++i) ids[i] = 4 * first + i;
  std::vector<WaveGroup> groups;
  const int form = fic_form(knobs_, fic_form_, soft_bits_ != 0, nblocks, ntiles);      // decoder_form.hpp; WAVE: rows per block and chunk of steps
  const bool wave_form = form == DABHIP_FORM_WAVE;
  fic_ran_ |= 1u << form;
  const int64_t dr = wave_form ? int64_t(64) * ((plan_table_[pid].nsteps + kWaveChunk - 1) / kWaveChunk) : (plan_table_[pid].nsteps + 7) / 8 * 8;
  for (int g = 0; g < ntiles; ++g) groups.push_back(WaveGroup{pid, 64 * g, std::min(64, nblocks - 64 * g), plan_table_[pid].nsteps, 0, g * dr});
  // The FIC kernels run on the side stream as well, behind what the main stream has queued so far (the FIC bits): 1008 waves of 774
  // steps fill a quarter of the chip's wave slots for 0.3 ms, so the main stream goes straight on with the rest of the OFDM stage
  // and the two share the GPU.  Everything that later touches these buffers on the main stream waits for the side stream
  // (ev_upload_ in decode_impl, the synchronising callers elsewhere).
  hipStream_t ks = copy;
  if (ks != stream_ && (!check(hipEventRecord(ev_fic_, stream_), "fic event") || !check(hipStreamWaitEvent(ks, ev_fic_, 0), "fic event"))) return false;
  {
    const std::vector<CodewordPlan>& plans = plan_table_.plans();
    if (!d_plans_.reserve(plans.size()) || !d_groups_.reserve(groups.size()) || !d_job_ids_.reserve(ids.size()) ||
        !d_grouped_.reserve(static_cast<size_t>(ntiles) * block_words * 64) || !d_decisions_.reserve(static_cast<size_t>(ntiles) * dr * 64))
      return false;
    const SmallUpload items[3] = {{plans.data(), d_plans_.get(), plans.size() * sizeof(CodewordPlan), false},
                                  {groups.data(), d_groups_.get(), groups.size() * sizeof(WaveGroup), false},
                                  {ids.data(), d_job_ids_.get(), ids.size() * sizeof(int), false}};
    if (!upload_small(items, 3, ks, h_small_fic_)) return false;
  }
  if (!check(launch_fic_group(d_fic_bits_.get(), 4 * first, nblocks, block_words, d_grouped_.get(), ks, limits_.fic_group_tiles, &report_.fic_group), "fic group launch") ||
      !check(launch_viterbi_form(form, soft_bits_, ViterbiLaunch{d_groups_.get(), ntiles, d_job_ids_.get(), d_plans_.get(), d_grouped_.get(), block_words,
                                                                 d_decisions_.get(), d_prbs_.get(), d_fibs_.get(), 96}, ks),
             "fic viterbi launch"))
    return false;
  if (!check(launch_fib_crc(d_fibs_.get() + static_cast<size_t>(first) * 384, n * 12, d_crc_tab_.get(), d_fib_ok_.get() + static_cast<size_t>(first) * 12, ks), "fib crc launch")) return false;
  if (!check(hipEventRecord(ev_fic_done_, ks), "fic event")) return false;
  // (few frames, page-locked destinations -- the engine's own: both downloads as one kernel that writes the host arrays itself, see scan_fetch)
  if (n <= 512 && fibs_host == h_fibs_.data() && ok_host == h_fib_ok_.data()) {
    HostWordsArgs hw{};
    hw.set(0, d_fibs_.get() + static_cast<size_t>(first) * 384, fibs_host, static_cast<size_t>(n) * 96);
    hw.set(1, d_fib_ok_.get() + static_cast<size_t>(first) * 12, ok_host, static_cast<size_t>(n) * 3);
    return check(launch_host_words(hw, copy), "fib download") && check(hipEventRecord(ev_fibs_, copy), "fib download event");
  }
  return check(hipMemcpyAsync(fibs_host, d_fibs_.get() + static_cast<size_t>(first) * 384, static_cast<size_t>(n) * 384, hipMemcpyDeviceToHost, copy), "fib download") &&
         check(hipMemcpyAsync(ok_host, d_fib_ok_.get() + static_cast<size_t>(first) * 12, static_cast<size_t>(n) * 12, hipMemcpyDeviceToHost, copy), "fib flag download") &&
         check(hipEventRecord(ev_fibs_, copy), "fib download event");
}

bool Engine::msc_prepare(const std::vector<const JobList*>& stream_jobs, const std::vector<const ControlPlane*>& planes,
                         const std::vector<int>& stream_row_base, const std::vector<int>& stream_fib_base, MscWork& out)
{
  const auto t_in = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) { host_mark("[host]   msc_prepare %-14s %8.3f ms\n", what, t_in); };
  std::string error;
  if (prepare_msc_work(plan_table_, *pool_, stream_jobs, planes, stream_row_base, stream_fib_base, limits_.decision_rows, out, &error, mark, msc_wave_max(knobs_, msc_form_)))
    return true;
  set_error(error);
  return false;
}

// work lists, ETI header bytes and frame records of a prepared batch to the device; `s` may be a side stream
bool Engine::msc_upload(const MscWork& w, hipStream_t s)
{
  if (w.nframes == 0) return true;
  if (!d_eti_.reserve(w.nframes * kEtiBytes)) return false;
  const DecodeBatch& b = w.batch;
  if (b.groups.empty())
    return d_meta_.upload(w.meta, s) && d_headers_.upload(w.headers, s) && d_stream_cif_base_.upload(w.stream_row_base, s);
  const std::vector<CodewordPlan>& plans = plan_table_.plans();
  const int row_words = kCifWords * (soft_bits_ ? 4 : 1);
  const size_t ntiles = b.job_ids.size() / 64;
  if (!d_meta_.reserve(w.meta.size()) || !d_headers_.reserve(w.headers.size()) || !d_stream_cif_base_.reserve(w.stream_row_base.size()) ||
      !d_plans_.reserve(plans.size()) || !d_groups_.reserve(b.groups.size()) || !d_job_ids_.reserve(b.job_ids.size()) || !d_jobs_.reserve(w.jobs.size()) ||
      !d_decisions_.reserve(static_cast<size_t>(b.max_dec_rows) * 64) || !d_grouped_.reserve(ntiles * row_words * 64))
    return false;
  // (the work lists are page-locked vectors -- MscWork --, the plan table and the row bases plain ones)
  const SmallUpload items[7] = {{w.meta.data(), d_meta_.get(), w.meta.size() * sizeof(EtiFrameMeta), true},
                                {w.headers.data(), d_headers_.get(), w.headers.size(), true},
                                {w.stream_row_base.data(), d_stream_cif_base_.get(), w.stream_row_base.size() * sizeof(int), false},
                                {plans.data(), d_plans_.get(), plans.size() * sizeof(CodewordPlan), false},
                                {b.groups.data(), d_groups_.get(), b.groups.size() * sizeof(WaveGroup), true},
                                {b.job_ids.data(), d_job_ids_.get(), b.job_ids.size() * sizeof(int), true},
                                {w.jobs.data(), d_jobs_.get(), w.jobs.size() * sizeof(DecodeJob), true}};
  return upload_small(items, 7, s, h_small_msc_);
}

// K4 + K5 queued on the main stream (nothing is awaited: the caller does that once, then msc_collect() reads the events)
bool Engine::msc_launch_async(const MscWork& w)
{
  const size_t nf = w.nframes;
  msc_queued_ = false;
  if (nf == 0) return true;
  // a fetch of the previous decode's frames may still be reading the ETI buffer these launches rewrite (eti_fetch_async)
  // (the newest fetch's event: the copies run in order on one stream.  Only while a fetch is outstanding: one that has been waited for has landed, and
  // a wait packet costs 10 .. 15 us of idle GPU in front of K4)
  if (const uint64_t issued = eti_fetch_issued_.load(); issued != eti_fetch_waited_.load())
    if (!check(hipStreamWaitEvent(stream_, ev_eti_fetch_[(issued - 1) & 1], 0), "eti fetch wait")) return false;
  if (!launch_decode_batch(w.batch, d_msc_bits_.get(), d_stream_cif_base_.get(), d_prbs_.get(), d_eti_.get(), kEtiBytes)) return false;
  if (!check(launch_eti_finish(d_meta_.get(), static_cast<int>(nf), d_headers_.get(), w.header_stride, d_fibs_.get(), d_crc_tab_.get(), d_crc_shift_.get(), d_eti_.get(), stream_), "eti finish launch"))
    return false;
  if (!record(ev_msc_[3], stream_)) return false;
  msc_queued_ = true;
  return true;
}

void Engine::msc_collect()
{
  if (!msc_queued_) return;
  msc_queued_ = false;
  float ms = 0;
  if (elapsed(&ms, ev_msc_[0], ev_msc_[1])) times_.gather += ms;
  if (elapsed(&ms, ev_msc_[1], ev_msc_[2])) times_.viterbi += ms;
  if (elapsed(&ms, ev_msc_[2], ev_msc_[3])) times_.eti += ms;
}

bool Engine::msc_launch(const MscWork& w)
{
  if (!msc_launch_async(w) || !check(hipStreamSynchronize(stream_), "msc decode")) return false;
  msc_collect();
  return true;
}

bool Engine::msc_run(MscWork& w) { return msc_upload(w, stream_) && msc_launch(w); }

}  // namespace dabhip
