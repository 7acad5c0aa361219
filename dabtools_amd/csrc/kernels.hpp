// kernels.hpp — host-callable launchers of the HIP kernels.  The tables of the Reed-Solomon launchers (gf_tables) are rs_code.hpp's GfRs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

#include "dabplus.hpp"
#include "device_types.hpp"
#include "dir.hpp"
#include "launch_limits.hpp"
#include "packet.hpp"
#include "ts.hpp"

namespace dabhip {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: several engines of one process may sit on different devices (dabhip_multi), each with
// its own host thread.  fn() runs once per device (the current one), its result is kept; callers on other threads of the same device wait for it.
template <class F>
inline hipError_t once_per_device(std::once_flag (&once)[64], hipError_t (&result)[64], F&& fn)
{
  int dev = 0;
  const hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  dev &= 63;
  std::call_once(once[dev], [&]() { result[dev] = fn(); });
  return result[dev];
}

// the scan's device-side preparation in one launch (k_sync.hip): h_* are page-locked host arrays the kernel reads directly
struct ScanSetupArgs {
  const StreamState* h_states;        // null: the device's states stay (a session's further segment)
  const uint8_t* const* h_ptrs;
  const int64_t* h_nbytes;
  const int* h_calls_before;
  StreamState* states;
  StreamState* states_prev;           // null unless the split scan runs (with calls_before and viol)
  const uint8_t** iq_ptrs;
  int64_t* nbytes;
  int* calls_before;
  int* viol;                          // nstreams + 1 entries
  uint4* descs;                       // cleared: desc_vec 16-byte pieces
  size_t desc_vec;
  uint4* info;
  size_t info_vec;
  int nstreams;
  uint8_t* tail_state;                // [nstreams][kTailBytes]: cleared with a fresh decode (h_states != null), kept in a session
  uint8_t* tail_state_prev;           // the incoming tail bytes, for a rescan (like states_prev)
};
hipError_t launch_scan_setup(const ScanSetupArgs& a, hipStream_t stream);
// up to four small arrays of 32-bit words from page-locked host memory to the device, and nzero words cleared, in one launch
struct HostWordsArgs {
  const uint32_t* src[4];
  uint32_t* dst[4];
  uint32_t nwords[4];
  uint32_t* zero;
  uint32_t nzero;
  void set(int k, const void* from, void* to, size_t n) { src[k] = static_cast<const uint32_t*>(from); dst[k] = static_cast<uint32_t*>(to); nwords[k] = static_cast<uint32_t>(n); }
};
hipError_t launch_host_words(const HostWordsArgs& a, hipStream_t stream);
// K1: synchronisation scan, one workgroup per stream, calls [call_begin, call_end) (call_end < 0: all).
// chain_only: FIFO bookkeeping, coarse and fine time only, assuming every frame's coarse frequency offset stays within +-1
// carrier; launch_sync_verify then computes both frequency estimates for all frames in parallel and records the first call
// of each stream that breaks the assumption.  states_in: where the incoming state is read from; stream_list: the streams to scan.
// tails: the streams' tail bytes (device_types.hpp: kTailBytes) -- carried in from state_in, out to state_out, one copy per call that reads a frame
// into images[(stream * max_calls + call) * kTailBytes] (FrameView::tail of that call's view points there); chunk: bytes appended per call (< 0: 262144)
struct SyncTails {
  const uint8_t* state_in;
  uint8_t* state_out;
  uint8_t* images;
  int chunk;
};
// The look-ahead schedule of a chain-only scan (small batches; k_sync.hip: sync_ahead_kernel): a pass that computes the chain's estimators for every call a
// stream has left, at every start position near the predicted one, all at once; the chain launch behind it looks them up.
struct SpecArgs {
  int2* table = nullptr;                // [nstreams][nspec][nhyp]: {null-symbol energy, fine time shift} of a read beginning at src0 + 2 (h - nhyp / 2); x < 0: none
  int64_t* src0 = nullptr;              // [nstreams][nspec]: predicted start position (stream offset) of the call's read, -1: no demodulating read expected
  int* ctl = nullptr;                   // [nstreams]: descriptor numbering of the scan (its first call), recorded by the launch with record_base; [nstreams]: table hits
  int nstreams = 0;
  int nspec = 0, nhyp = 0;
  int lookup = 0;                       // chain launches: the table stands for the calls from where the stream stands now
  int call_limit = -1;                  // chain launches: at most this many calls per stream (< 0: to the end)
  int record_base = 0;
};
// What every K1 launch shares: the streams' samples and sizes, their front-end states, the calls' descriptors (descs[stream * max_calls + call]) and
// {status, ordinal} records, the fp64 twiddles and the phase reference symbol.
struct SyncArgs {
  const uint8_t* const* iq; const int64_t* nbytes; StreamState* states; CallDesc* descs; int2* info; int nstreams, max_calls;
  const double2 *tw2048, *tw1536; const uint8_t* prs_q;
};
// ... and what differs from one scan launch to the next
struct SyncScanOpts {
  int call_begin = -1, call_end = -1;     // the calls to run (call_end < 0: all)
  int afc = 0;
  bool chain_only = false;
  const StreamState* states_in = nullptr; // null: a.states
  const int* stream_list = nullptr;       // null: block b = stream b; else the a.nstreams streams to scan
  SyncTails tails{nullptr, nullptr, nullptr, -1};
  SpecArgs spec;
};
hipError_t launch_sync_scan(const SyncArgs& a, const SyncScanOpts& o, hipStream_t stream);
// the look-ahead pass over the calls every stream has left from where it stands (at most spec.nspec of them)
hipError_t launch_sync_ahead(const SyncArgs& a, const SpecArgs& spec, hipStream_t stream);
// carry_only = false: the verification pass (violation[b] = first offending call, untouched otherwise);
// carry_only = true: fine_freq_shift carried through the calls that did not demodulate, for the streams without a violation
hipError_t launch_sync_verify(const SyncArgs& a, const int* calls_before, int* violation, bool carry_only, hipStream_t stream);

// What every launch over the frame list shares: the streams' samples, the calls' descriptors (descs[stream * max_calls + call]), the list itself
// (frames[i] = {stream, call}, FIC rows at TF slot frame_slot[i], MSC rows from logical CIF row frame_cif_row[i]), the fp32 twiddles, the
// carrier -> QPSK symbol map and the bit rows.  Such a launch covers frames [first, first + nframes) of the list.
struct FrameListArgs {
  const uint8_t* const* iq; const CallDesc* descs; int max_calls; const int2* frames; const float2* tw;
  const int *frame_slot, *frame_cif_row; const uint16_t* qpsk_of_carrier; uint32_t *fic_bits, *msc_bits;
};

// delta != nullptr: the kernel also leaves the guard's per-symbol error bound delta_c sqrt(sum |x|^2) at delta[(first + j) * 76 + symbol]
// (delta_c = GuardArgs::c of the launches that will read it: the guard level's constant, or kSoftNormC for soft decisions)
hipError_t launch_ofdm_fft(const FrameListArgs& f, int first, int nframes, float2* spectra, hipStream_t stream, float* delta = nullptr, float delta_c = kGuardC);

// K2b: DQPSK + demap + frequency de-interleave -> bit-packed rows.  FIC rows at TF slot frame_slot[first + j];
// MSC rows start at CIF row frame_cif_row[first + j]: planar = scattered into time-de-interleaved logical rows
// (see k_fft.hip), else the four transmitted CIFs of the TF in natural bit order.
hipError_t launch_demap(bool planar, int soft_bits, const float2* spectra, int first, int nframes, const int* frame_slot,
                        const int* frame_cif_row, const uint16_t* qpsk_of_carrier, uint32_t* fic_bits, uint32_t* msc_bits,
                        const GuardArgs& guard, hipStream_t stream);

// FIC pre-pass: DFT of symbols 0..3 of every frame + demap of the three FIC symbols (spectra4: [nframes][4][2048])
hipError_t launch_fic_prepass(int soft_bits, const FrameListArgs& f, int first, int nframes, float2* spectra4, const GuardArgs& guard, hipStream_t stream);

// S1 seam: Viterbi on explicit per-step symbol bytes (forward pass + chain-back + pack)
hipError_t launch_viterbi(const WaveGroup* groups, int ngroups, const int* job_ids, const CodewordPlan* plans, const uint4* steps,
                          uint2* decisions, const uint32_t* prbs_words, uint8_t* out, int record_stride, hipStream_t stream);

// K3/K4: lane-interleave the received rows 64 records at a time (soft_bits: 0 = hard bits, 4 = 4-bit soft values),
// then Viterbi with fused de-puncturing
// (max_tiles: tiles per launch, launch_limits.hpp -- a multiple of 8 for the regroup; launches: counts the launches made, when not null)
hipError_t launch_regroup(int soft_bits, const int* job_ids, int ntiles, const DecodeJob* jobs, const int* stream_cif_base,
                          const uint32_t* rows, uint32_t* grouped, hipStream_t stream, int max_tiles = kMaxRegroupTiles, int64_t* launches = nullptr);
hipError_t launch_fic_group(const uint32_t* fic_rows, int first_block, int nblocks, int block_words, uint32_t* grouped, hipStream_t stream,
                            int max_tiles = kMaxFicGroupTiles, int64_t* launches = nullptr);
// One launch of the decoder over ngroups wave-groups (worklist.hpp), whatever its form: rows of row_words words per record in `grouped`, survivor
// records in `decisions`, decoded bytes de-scrambled with prbs_words into out + record * record_stride.
struct ViterbiLaunch {
  const WaveGroup* groups; int ngroups; const int* job_ids; const CodewordPlan* plans; const uint32_t* grouped; int row_words;
  uint2* decisions; const uint32_t* prbs_words; uint8_t* out; int record_stride;
};
// form: DABHIP_FORM_WAVE / LANE / TWO_PLAIN / FOUR (hard and soft decisions) / TWO (hard only: hipErrorInvalidValue with soft_bits); decoder_form.hpp has the rule
hipError_t launch_viterbi_form(int form, int soft_bits, const ViterbiLaunch& v, hipStream_t stream);

// The low-latency form of the same decoder (k_vitwave.hip): one WAVE per code word, lane = trellis state -- a fraction of the fused kernel's
// time per code word at four times its lane-ops, for small batches.  Same groups / plans / rows / output; decisions: rows of 64 x 8 bytes, one per
// code word and chunk of kWaveChunk steps: group g's 64 x ceil(nsteps / kWaveChunk) rows start at groups[g].dec_base.
constexpr int kWaveChunk = 60;

// the one-kernel OFDM stage (k_fused.hip, compiled three times): with the parity guard's test in its symbol loop, without it, and
// with 4-bit soft values instead of hard decisions.
// Data symbols [sym_a, sym_b) of every frame (1..3 = FIC, 4..75 = MSC), nparts workgroups per frame; each transforms the symbol before
// its first data symbol as differential reference.
hipError_t launch_ofdm_demap_fused_guarded(const FrameListArgs& f, int first, int nframes, const GuardArgs& guard, hipStream_t stream, int sym_a = 1, int sym_b = 76,
                                           int nparts = 4);
// the guarded kernel's audit build (k_fused.hip with -DDABHIP_FUSED_AUDIT=1): also leaves dump_bins[frame][76][2048] (by raw bin) and
// dump_prod[frame][76][2048] ((re, im) of cur conj(prev) of the data symbols as the kernel computed them)
hipError_t launch_ofdm_demap_fused_audit(const FrameListArgs& f, int first, int nframes, const GuardArgs& guard, hipStream_t stream, int sym_a, int sym_b, int nparts,
                                         float2* dump_bins, float2* dump_prod);
hipError_t launch_ofdm_demap_fused_soft(bool afc, const FrameListArgs& f, int first, int nframes, hipStream_t stream, int sym_a = 1, int sym_b = 76, int nparts = 4);
hipError_t launch_ofdm_demap_fused_plain(bool afc, const FrameListArgs& f, int first, int nframes, hipStream_t stream, int sym_a = 1, int sym_b = 76, int nparts = 4);
// parity guard (k_parity.hip): per-symbol error bounds, fp64 re-decision of the flagged carriers, and the audit
hipError_t launch_symbol_delta(const FrameListArgs& f, int first, int nframes, int nsym, float* delta, int delta_stride, float delta_c, hipStream_t stream);
hipError_t launch_exact_decide(const uint4* list, const unsigned* counter, unsigned cap, const FrameListArgs& f, const double2* tw2048, bool planar, hipStream_t stream);
// list overflow of a guarded launch: its frames' symbols [sym_a, sym_b) decided again in full from fp64 transforms (returns at once otherwise)
hipError_t launch_exact_decide_all(const unsigned* counter, unsigned cap, const FrameListArgs& f, int first, int nframes, int sym_a, int sym_b, const double2* tw2048,
                                   bool planar, bool skip_fic, hipStream_t stream);
hipError_t launch_decision_audit(const uint8_t* frames_iq, int nframes, const float2* spectra, const uint32_t* fic_bits, const uint32_t* msc_bits,
                                 const double2* tw2048, const uint16_t* qpsk_of_carrier, void* out, hipStream_t stream,
                                 const float2* fused_prods = nullptr, int row_lead = 0, int guard_level = 1);   // fused_prods != null: the fused kernel's audit (spectra = its bins by raw bin)
hipError_t launch_batched_copy(const CopyDesc* descs, int n, hipStream_t stream);
// the descriptors' sources may be page-locked HOST memory (read over PCIe by a small persistent grid); nbytes < 4 GiB each
hipError_t launch_host_gather(const CopyDesc* descs, int n, int workgroups, hipStream_t stream);
// n copies inside the device in one launch per max_descs of them (at most 65535: grid.y), any alignment; max_bytes = the longest of them
hipError_t launch_device_gather(const CopyDesc* descs, int n, uint32_t max_bytes, hipStream_t stream, int max_descs = kMaxGatherDescs, int64_t* launches = nullptr);
hipError_t launch_fib_crc(const uint8_t* fibs, int nfib, const uint16_t* crc_tab, uint8_t* ok, hipStream_t stream);

// K5: ETI header/FIB copy, EOF CRC, trailer
hipError_t launch_eti_finish(const EtiFrameMeta* meta, int nframes, const uint8_t* headers, int header_stride, const uint8_t* fibs,
                             const uint16_t* crc_tab, const uint16_t* shift_cols, uint8_t* eti, hipStream_t stream);

// k_dabplus.hip: DAB+ superframes out of ETI frames (dabplus.hpp has the types, dabhip.h the sync rule).  locate: the sub-channels of every
// (stream, frame) into loc [nstreams][maxv][nsub]; sync + scan + jobs: the candidates of every (stream, sub-channel) (at most cap each), the push's
// superframe list, totals = {superframes, codewords}; rs: the ncw codewords into data (110 s bytes per superframe) and cw_status (symbols
// corrected, 0xff = failed), gf_tables: a GfRs<kRsRoots> filled by rs_tables_fill (rs_code.hpp), syn: 16 bytes of scratch per codeword; au: one
// record per superframe and the counters (crc_tab: the CRC-16 byte table, then x^(8 n) mod G for n < kRsK kMaxS; data: 16 bytes of slack at its
// end); carry: the last 4 frames of every stream.
hipError_t launch_dabplus_locate(const DabPlusFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, DabPlusLoc* loc, hipStream_t stream);
hipError_t launch_dabplus_sync(const DabPlusFrames& fr, int nstreams, int nsub, int maxv, const DabPlusLoc* loc, DabPlusSync* sync, DabPlusCand* cand,
                               int cap, int* ncand, int* lane_cw, int64_t* counters, DabPlusJob* jobs, int* lane_sf_base, int* lane_cw_base, int* totals,
                               hipStream_t stream);
hipError_t launch_dabplus_rs(const DabPlusJob* jobs, const int* totals, int ncw, const DabPlusLoc* loc, int maxv, int nsub, const uint8_t* gf_tables,
                             uint8_t* data, uint8_t* cw_status, uint32_t* syn, hipStream_t stream);
hipError_t launch_dabplus_au(const DabPlusJob* jobs, int nsf, const DabPlusLoc* loc, int maxv, int nsub, const uint8_t* data, const uint8_t* cw_status,
                             const uint16_t* crc_tab, dabhip_dabplus_sf* recs, int64_t* counters, hipStream_t stream);
hipError_t launch_dabplus_carry(const DabPlusFrames& fr, int nstreams, uint8_t* carry_next, hipStream_t stream);

// k_packet.hip: packet-mode data out of ETI frames (packet.hpp has the types and the sync rule, dabhip.h the rules in words).  locate: the
// sub-channels of every (stream, new frame) into loc [nstreams][maxv][nsub]; sync + scan + jobs: every lane's virtual cell numbering, its units (at
// most cap each) and the push's unit list, totals = {units, buffer cells}; gather: the units' cells into the cell buffer; rs: the 12 code words of
// every RS-decoded frame, corrected in place (gf_tables: a GfRs<kPkRoots> filled by rs_tables_fill; cw_status: symbols corrected, 0xff = failed;
// syn: 16 bytes of scratch per code word); cand: per
// buffer cell, the length of the packet the walk may take there (crc_tab: the CRC-16 byte table); walk: a record per buffer cell (length 0: none)
// and the counters; carry: every lane's unconsumed cells (at most 102).
hipError_t launch_packet_locate(const EtiFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, PacketLoc* loc, hipStream_t stream);
hipError_t launch_packet_sync(const EtiFrames& fr, int nstreams, int nsub, int maxv, const uint8_t* fec, PacketLoc* loc, PacketSync* sync, const uint8_t* carry,
                              PacketSlot* slots, int cap, int* nunits, int* lane_buf, int* ncar_in, int* ncar_out, int* lo, int64_t* counters, PacketUnit* units,
                              int* lane_unit_base, int* lane_buf_base, int* totals, hipStream_t stream);
hipError_t launch_packet_gather(const EtiFrames& fr, const PacketUnit* units, const int* totals, int ncells, const PacketLoc* loc, int maxv, int nsub,
                                const uint8_t* carry, const int* ncar_in, uint8_t* cells, hipStream_t stream);
hipError_t launch_packet_rs(const PacketUnit* units, const int* totals, int nunits, const uint8_t* gf_tables, uint8_t* cells, uint8_t* cw_status, uint32_t* syn,
                            hipStream_t stream);
hipError_t launch_packet_cand(const PacketUnit* units, const int* totals, int ncells, const uint16_t* crc_tab, const uint8_t* cells, uint8_t* cand, hipStream_t stream);
hipError_t launch_packet_walk(const PacketUnit* units, const int* totals, int nunits, const uint8_t* cells, const uint8_t* cand, const uint8_t* cw_status,
                              dabhip_packet_rec* recs, int64_t* counters, int* npackets, hipStream_t stream);
hipError_t launch_packet_carry(const EtiFrames& fr, int nlanes, const PacketLoc* loc, int maxv, int nsub, const uint8_t* carry, const int* ncar_in,
                               const int* ncar_out, const int* lo, uint8_t* carry_next, hipStream_t stream);

// k_ts.hip: MPEG-2 TS packets out of ETI frames (ts.hpp has the types, ts_sync.hpp the sync rule and the position map, dabhip.h the rules in
// words).  locate (+ layout): the sub-channels of every (stream, new frame) into loc [nstreams][maxv][nsub], every lane's virtual positions and
// its words in the run-flag buffer (flag_cap words; totals zeroed before); runs: a bit per position, "a run of five starts here"; sync: a wave per
// lane, its units into at most cap slots; jobs (scan + jobs): the push's unit list, totals[0] = units; gather: the units' 204 bytes into the word
// buffer (ts_word_byte); syndrome / decode: the code words, corrected in place (cw_status: symbols corrected, 0xff = failed; syn: 16 bytes of
// scratch per code word; gf_tables as the packet stage's); parse: a record and 188 bytes per unit, the counters; carry: every lane's
// unconsumed bytes (at most 2447).
hipError_t launch_ts_locate(const EtiFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, TsLoc* loc, const TsSync* sync, TsLane* lanes, int flag_cap,
                            int* totals, hipStream_t stream);
hipError_t launch_ts_runs(const EtiFrames& fr, int nlanes, int nsub, int maxv, int per_lane, const TsLoc* loc, const TsLane* lanes, const uint8_t* carry,
                          const int* totals, uint64_t* flags, hipStream_t stream);
hipError_t launch_ts_sync(const EtiFrames& fr, int nlanes, int nsub, int maxv, const TsLoc* loc, TsSync* sync, TsLane* lanes, const uint8_t* carry,
                          const uint64_t* flags, TsSlot* slots, int cap, int* nunits, int64_t* counters, int* totals, hipStream_t stream);
hipError_t launch_ts_jobs(int nlanes, const TsSlot* slots, int cap, const int* nunits, int* lane_unit_base, const TsSync* sync, const TsLane* lanes, TsUnit* units,
                          int64_t unit_cap, int* totals, hipStream_t stream);
hipError_t launch_ts_gather(const EtiFrames& fr, const TsUnit* units, const int* totals, int64_t nunits, const TsLoc* loc, int maxv, int nsub, const uint8_t* carry,
                            const TsLane* lanes, uint8_t* words, hipStream_t stream);
hipError_t launch_ts_syndrome(const int* totals, int64_t nunits, const uint8_t* gf_tables, const uint8_t* words, uint8_t* cw_status, uint32_t* syn, hipStream_t stream);
hipError_t launch_ts_decode(const int* totals, int64_t nunits, const uint8_t* gf_tables, uint8_t* words, uint8_t* cw_status, const uint32_t* syn, hipStream_t stream);
hipError_t launch_ts_parse(const TsUnit* units, const int* totals, int64_t nunits, const uint8_t* words, const uint8_t* cw_status, dabhip_ts_rec* recs, uint8_t* data,
                           int64_t* counters, hipStream_t stream);
hipError_t launch_ts_carry(const EtiFrames& fr, int nlanes, const TsLoc* loc, int maxv, int nsub, const uint8_t* carry, const TsLane* lanes, const int* totals,
                           uint8_t* carry_next, hipStream_t stream);

// k_dir.hip: the ensemble directory out of ETI frames (dir.hpp has the types, dir_figs.hpp the rules, dabhip.h the rules in words).  fibs: a thread
// per (stream, new frame, FIB): frame header, CRC, FIG walk; its facts into the FIB's kDirFactSlots slots of `facts` and its DirFib record, both
// indexed by (base[s] + frame) * 3 + fib.  merge: a wave per stream applies the stream's facts in order to its tables (staged in LDS), adds its
// counters and leaves the FIBs of this push whose CRC held in ok_fibs[s].
hipError_t launch_dir_fibs(const EtiFrames& fr, int nstreams, int maxv, DirFib* fibs, DirFact* facts, hipStream_t stream);
hipError_t launch_dir_merge(const EtiFrames& fr, int nstreams, const DirFib* fibs, const DirFact* facts, DirStream* state, int* ok_fibs, hipStream_t stream);

// k_probe.hip: streaming rates of this device (fill, copy, K2's read/write mix) in GB/s -- bench.py's yardstick beside the K2 figure
int stream_ceiling(int device, size_t bytes, int reps, double* gbs);

}  // namespace dabhip
