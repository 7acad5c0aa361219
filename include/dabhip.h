/*
 * dabhip.h — C ABI of libdabhip.so, the MI355X-native DSP back end for dab2eti.
 *
 * Plain C, caller-owned buffers, int error codes (0 = ok, <0 = error, see
 * dabhip_last_error()).  No C++ or torch types cross this boundary.
 *
 * The reference (linuxstb/dabtools) has no plugin system; its seams are C function
 * signatures chosen at link time.  Each entry point below names the reference interface
 * (file:line under src/) it replaces.  INTEGRATION.md shows the reference-side binding.
 *
 *   S1  decoder seam      viterbi.h:6-8, viterbi_spiral.h:22-23   -> dabhip_*viterbi*
 *   S2  front-end seam    input_sdr.h:43-44                        -> dabhip_sdr_*
 *   S3  back-end seam     dab.h:91-92 (+ eti_callback dab.h:88)    -> dabhip_dab_*
 *   batch engine (new: B independent ensembles resident in HBM)    -> dabhip_engine_*
 *   stage entries for parity tests                                 -> dabhip_stage_*
 *   synthetic Mode-I modulator (workload generator; host, or on the GPU) -> dabhip_synth_*
 */
#ifndef DABHIP_H
#define DABHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DABHIP_TF_BYTES 393216        /* one transmission frame of cu8 IQ (input_sdr.h:16) */
#define DABHIP_CHUNK_BYTES 262144     /* DEFAULT_BUF_LENGTH, input_sdr.h:9 */
#define DABHIP_FIC_BITS 9216          /* fic_symbols_demapped[3][3072], dab.h:29 */
#define DABHIP_MSC_BITS 221184        /* msc_symbols_demapped[72][3072], dab.h:32 */
#define DABHIP_ETI_BYTES 6144         /* dab2eti.c:132-135 */

/* ---- library ------------------------------------------------------------------------ */
const char *dabhip_last_error(void);          /* thread-local text of the last failure */
int dabhip_device_count(void);                /* number of visible HIP devices (0 without a GPU) */

/* ---- S1: decoder seam ---------------------------------------------------------------- */
/* Replaces init_viterbi() (viterbi.h:6, viterbi.c:455) / create_viterbi(len)
 * (viterbi_spiral.h:22).  Returns an opaque handle (never NULL on success). */
void *dabhip_create_viterbi(int len);
int dabhip_init_viterbi(void);
/* Replaces viterbi(p, symbols, data, framebits) (viterbi.h:8, viterbi.c:352-451; called
 * from fic.c:186 and misc.c:262).  symbols: 4*(framebits+6) bytes, 127/129 hard values,
 * 128 = erasure (depuncture.c:36-43).  data: (framebits+7)/8 bytes, MSB first.  Decisions
 * are those of the scalar reference decoder (metrics 3/-7/0, ties keep the low
 * predecessor).  p may be NULL (uses a process-wide engine on device 0). */
void dabhip_viterbi(void *p, unsigned char *symbols, unsigned char *data, int framebits);
/* Batch form: n code words of equal length, symbols packed back to back. */
int dabhip_viterbi_batch(void *p, const unsigned char *symbols, unsigned char *data, int framebits, int n);

/* ---- S2: front-end seam --------------------------------------------------------------- */
typedef struct dabhip_sdr dabhip_sdr;
/* Replaces sdr_init(struct sdr_state_t*) (input_sdr.h:44, input_sdr.c:167-186). */
dabhip_sdr *dabhip_sdr_init(int device);
void dabhip_sdr_free(dabhip_sdr *s);
/* Replaces sdr_demod(tf, sdr) (input_sdr.h:43, input_sdr.c:27-165).  input_buffer /
 * input_buffer_len are what rtlsdr_callback stores in sdr->input_buffer (dab2eti.c:125-126).
 * On return 1 the two arrays hold tf->fic_symbols_demapped (9216 bytes of 0/1) and
 * tf->msc_symbols_demapped (221184 bytes of 0/1); on return 0 they are untouched.
 * <0 = error. */
int dabhip_sdr_demod(dabhip_sdr *s, const uint8_t *input_buffer, int input_buffer_len,
                     uint8_t *fic_symbols_demapped, uint8_t *msc_symbols_demapped);
/* The side-channel outputs dab2eti.c:76-103 reads after each call. */
int32_t dabhip_sdr_coarse_timeshift(const dabhip_sdr *s);
int32_t dabhip_sdr_fine_timeshift(const dabhip_sdr *s);
int32_t dabhip_sdr_coarse_freq_shift(const dabhip_sdr *s);
double dabhip_sdr_fine_freq_shift(const dabhip_sdr *s);

/* ---- S3: back-end seam ---------------------------------------------------------------- */
typedef struct dabhip_dab dabhip_dab;
typedef void (*dabhip_eti_callback)(uint8_t *eti);                    /* dab.h:88 */
typedef void (*dabhip_eti_sink)(const uint8_t *eti, int stream, void *user);
/* Replaces init_dab_state(&dab, device_state, eti_callback) (dab.h:91, dab.c:14-33). */
dabhip_dab *dabhip_dab_init(int device, dabhip_eti_callback cb);
void dabhip_dab_free(dabhip_dab *d);
/* The caller fills these before each dabhip_dab_process_frame(), exactly as sdr_demod
 * fills dab->tfs[dab->tfidx] (dab2eti.c:68). */
uint8_t *dabhip_dab_tf_fic(dabhip_dab *d);   /* 9216 bytes */
uint8_t *dabhip_dab_tf_msc(dabhip_dab *d);   /* 221184 bytes */
/* Replaces dab_process_frame(dab) (dab.h:92, dab.c:35-98): invokes the callback 0 or 4
 * times, synchronously, with a pointer to a 6144-byte frame valid during the call.
 * Sub-channels of every size are decoded: all that fit the CIF and the ETI frame (see dabhip_engine_stream_status), up to 43,782 trellis steps and
 * 5,472 bytes per CIF (EEP 4-B at n = 57).  Above 13,824 data bits per code word -- EEP A levels beyond n = 72, B levels beyond n = 18 -- the
 * reference's own decoder is past its allocation (create_viterbi(768*18), dab.c:29): parity there is with the oracle and with the transmitted payload. */
int dabhip_dab_process_frame(dabhip_dab *d);
int dabhip_dab_locked(const dabhip_dab *d);
/* What the reference's dab_process_frame prints on stderr for its operator -- "Locked" (dab.c:51), "Lock lost, resetting ringbuffer" (dab.c:57), the one-time
 * ensemble dump (dab.c:78-82, misc.c:316-328) -- as text: what is pending since the last call is copied to buf (NUL-terminated, cut at cap - 1 bytes) and
 * cleared; returns the pending text's length (0: nothing happened), < 0: bad handle.  integration/dab_hip.c writes it to stderr. */
int64_t dabhip_dab_take_log(dabhip_dab *d, char *buf, int64_t cap);
/* as dabhip_engine_stream_status for this seam: with a flagged multiplex dabhip_dab_process_frame invokes the callback 0 times where
 * dab_process_frame (dab.c:85-95 -> misc.c:218-314) would run off its arrays */
uint32_t dabhip_dab_status(const dabhip_dab *d);
/* Soft-decision extension of this seam (not in the reference: dab.h:27-33 carries 0/1 bytes): after dabhip_dab_set_soft(d, 1) --
 * before the first frame only -- the two arrays carry signed 4-bit values as int8 (-7 .. 7; > 0: the hard bit would be 0; the
 * demapper's rule is dabhip_engine_set_soft's) and the FIC / MSC decoders use them as branch metrics.  Lets a test feed the
 * decoders the very values an independent restatement decodes (oracle/or_soft.c). */
int dabhip_dab_set_soft(dabhip_dab *d, int enable);
/* Decoder forms of this seam (dabhip_engine_set_decoder_forms, DABHIP_FORM_*; any time); the report covers the last dabhip_dab_process_frame. */
int dabhip_dab_set_decoder_forms(dabhip_dab *d, int msc_form, int fic_form);
int dabhip_dab_set_soft_lanes(dabhip_dab *d, int enable);   /* dabhip_engine_set_soft_lanes for this seam; any time */
int dabhip_dab_decoder_forms(const dabhip_dab *d, uint32_t *msc_mask, uint32_t *fic_mask);
/* launch limits and the last process_frame's launches: see dabhip_engine_set_launch_limits */
int dabhip_dab_set_launch_limits(dabhip_dab *d, const int64_t *limits, int n);
int dabhip_dab_launch_report(const dabhip_dab *d, int64_t *out, int cap);
/* FIBs (12 x 32 bytes) and CRC flags (12) of the TF processed last (struct tf_fibs_t, dab.h:21-25). */
int dabhip_dab_last_fibs(const dabhip_dab *d, uint8_t *fibs, uint8_t *crc_ok);

/* ---- batch engine ---------------------------------------------------------------------- */
typedef struct dabhip_engine dabhip_engine;
dabhip_engine *dabhip_engine_create(int device);
/* The same with an explicit size for the engine's host thread pool (per-stream control plane, work lists, staging copies);
 * 0 = automatic (half the cores, at most 24).  Several engines in one process should share the host between them. */
dabhip_engine *dabhip_engine_create_ex(int device, int host_threads);
/* The same with the engine's host threads bound to the listed CPUs (ncpus = 0: to the CPUs of the device's NUMA node on a machine with several,
 * else unbound).  dabhip_engine_host_cpus reports what was applied. */
dabhip_engine *dabhip_engine_create_on_cpus(int device, int host_threads, const int32_t *cpus, int ncpus);
int dabhip_engine_host_cpus(const dabhip_engine *e, int32_t *cpus, int cap, int *numa_node);
void dabhip_engine_destroy(dabhip_engine *e);

/* Decode B independent cu8 streams (the replay loop of dab2eti.c:60-130 per stream, in
 * 262144-byte chunks, trailing partial chunk dropped).  iq[b] are DEVICE pointers when
 * on_device != 0, host pointers otherwise.  ETI frames stay in device memory; query
 * them with the calls below.  Returns total ETI frames produced, <0 on error. */
int64_t dabhip_engine_decode(dabhip_engine *e, const uint8_t *const *iq, const size_t *nbytes, int nstreams,
                             int on_device);
int64_t dabhip_engine_eti_count(const dabhip_engine *e, int stream);      /* frames of one stream */
/* Per-stream status of the last decode (fault isolation).  The FIC carries a 16-bit CRC and fib_parse (fic.c:47-130) validates nothing: a corrupted
 * FIB that passes the CRC can signal a multiplex the reference cannot assemble inside its own arrays -- create_eti then writes past eti[6144]
 * (misc.c:233,246-296), uep_/eep_depuncture read past cif_time_deinterleaved[55296] (depuncture.c:84-132), eeptable[] is indexed past its 8 rows
 * (fic.c:84): undefined behaviour, no parity target.  Here such a stream is flagged and emits NO frames while its multiplex is in that state (for
 * good: the reference only ever adds sub-channels, misc.c:14-21); lock rule, CIF ring and frame counter move on as they would; every other stream
 * of the batch decodes exactly as if it were alone.  0 = fine; 0xffffffff = no such stream.
 * A multiplex that raises none of the flags is decoded whatever the sizes of its sub-channels, one that fills all 864 capacity units included; above
 * 13,824 data bits per code word the reference's decoder is past its own allocation (dab.c:29) and parity is with the oracle and the transmitted payload.
 * Under a sub-channel filter (dabhip_engine_set_subchannels) the flags describe the CARRIED multiplex, the listed sub-channels alone: a sub-channel
 * that is not listed is neither decoded nor placed in the frame, so what the FIC says of it raises no flag and silences nothing -- the stream's status
 * stays 0 and its frames keep coming, with the FIC passed on as received.  Listed, the same sub-channel raises the flags of the unfiltered decode. */
#define DABHIP_STREAM_MUX_OVERFLOW 1u       /* header + FIC + sub-channel bytes + trailer exceed 6144 bytes */
#define DABHIP_STREAM_SUBCH_OUTSIDE_CIF 2u  /* a sub-channel's transmitted bits end beyond capacity unit 863 */
#define DABHIP_STREAM_EEP_OPTION 4u         /* EEP protection option > 1: outside ETSI EN 300 401 and past the reference's table */
#define DABHIP_STREAM_SUBCH_SIZE 8u         /* EEP size below one unit of its level (bit rate 0): the reference's frame carries uninitialised stack bytes there */
uint32_t dabhip_engine_stream_status(const dabhip_engine *e, int stream);
/* The reference's operator feedback for one stream of the last decode: what dab_process_frame prints on stderr -- "Locked" (dab.c:51), "Lock lost,
 * resetting ringbuffer" (dab.c:57), the one-time ensemble dump "ENSEMBLE_INFO: ..." / "SubChId=..." (dab.c:78-82, misc.c:316-328) -- same text, same
 * order.  The text pending since the last call is copied to buf (NUL-terminated, cut at cap - 1 bytes) and cleared; returns its full length (0: nothing
 * to report), < 0: no such stream.  dab2eti-hip prints it on stderr. */
int64_t dabhip_engine_stream_log(dabhip_engine *e, int stream, char *buf, int64_t cap);
/* Copy the ETI frames of one stream (in emission order) to host memory. */
int64_t dabhip_engine_eti_read(dabhip_engine *e, int stream, uint8_t *dst, int64_t cap_frames);
/* Deliver all frames, stream by stream in emission order, to a sink (stdout contract helper). */
int64_t dabhip_engine_eti_drain(dabhip_engine *e, dabhip_eti_sink sink, void *user);
const void *dabhip_engine_eti_device_ptr(const dabhip_engine *e, int64_t *nframes); /* all frames, stream-major */
/* The output leg of the CLI contract (eti_callback -> write(1, eti, 6144), dab2eti.c:132-135) without a stall: ALL frames of the last decode,
 * stream by stream in emission order (the order dabhip_engine_eti_drain delivers them in), copied to dst -- page-locked memory from
 * dabhip_host_alloc for a true asynchronous DMA -- on a stream of their own.  Returns at once with the number of frames on their way (<= cap_frames);
 * the copy runs beside the NEXT decode (only that decode's ETI-writing launches wait for it); dabhip_engine_eti_fetch_wait returns when the
 * bytes have arrived.  dst must stay untouched in between.  At most TWO fetches may be outstanding (two output buffers: one being written out
 * while the next fills); each dabhip_engine_eti_fetch_wait waits for the OLDEST fetch not yet waited for, and a third fetch without a wait is
 * refused (-1).  The waiting thread may be another one than the decoding thread (the CLI's writer thread). */
int64_t dabhip_engine_eti_fetch(dabhip_engine *e, uint8_t *dst, int64_t cap_frames);
int dabhip_engine_eti_fetch_wait(dabhip_engine *e);

/* Software AFC (beyond the reference's file-less operation): when enabled every stream gets an NCO
 * steered by the tuner feedback rule of dab2eti.c:76-103 (coarse offset > 1 carrier: +-1000 Hz; = 1: a random step
 * below 1000 Hz; else fine estimate / 3 when above 50 Hz), so captures with a carrier frequency offset decode without a
 * tuner.  Default off = parity mode (samples untouched, results identical to the reference). */
int dabhip_engine_set_afc(dabhip_engine *e, int enable);

/* Soft-decision decoding (BASELINE config 5; the reference decodes hard decisions only,
 * input_sdr.c:157-158, depuncture.c:36-43): the demapper emits signed 4-bit values that travel through time
 * de-interleaving and de-puncturing into the Viterbi branch metrics of FIC and MSC.  Batch engine only.  Default off =
 * parity mode (bit-exact with the reference).  With soft decisions the output equals the reference's wherever that decodes
 * without errors and is better (lower BER) at low SNR. */
int dabhip_engine_set_soft(dabhip_engine *e, int enable);

/* Viterbi decoder forms (test plumbing: which kernel decodes is otherwise chosen by batch size, engine.hpp; the bytes are the same in every form).
 * MSC: DABHIP_FORM_WAVE       one wave per code word (k_vitwave.hip; the default up to 12,288 code words)
 *      DABHIP_FORM_LANE       one lane per code word (viterbi_fused_kernel; the default above 1,536 groups of 64 code words)
 *      DABHIP_FORM_TWO        two lanes per code word (vit_two_lanes.hpp; the default from 801 to 1,536 groups)
 *      DABHIP_FORM_TWO_PLAIN  two lanes per code word, table-free (vit_four_lanes.hpp; otherwise only with DABHIP_VIT_LANES_PLAIN=1)
 *      DABHIP_FORM_FOUR       four lanes per code word (vit_four_lanes.hpp; the default up to 800 groups)
 * FIC: DABHIP_FORM_WAVE (default up to 3,072 blocks), DABHIP_FORM_LANE, DABHIP_FORM_FOUR (default up to 128 tiles of 64 blocks).
 * dabhip_engine_set_decoder_forms sets the form of every MSC and every FIC launch of the engine, over the environment knobs
 * (DABHIP_VIT_WAVE_MAX and its kin); DABHIP_FORM_AUTO restores the rule of the knobs and defaults.  -1 with error text for a
 * form the decoder does not have (TWO and TWO_PLAIN for the FIC).  A forced WAVE decodes every batch in one launch (the lane forms split a launch
 * past 24 GiB of survivor records).
 * Soft decisions (dabhip_engine_set_soft) and the multi-lane forms, by dabhip_engine_set_soft_lanes (default off; DABHIP_SOFT_LANES=1):
 *   off: the multi-lane forms take hard decisions only.  A soft launch outside the wave form runs the lane form; a forced TWO, TWO_PLAIN or FOUR
 *        runs the lane form too, and the report says LANE.
 *   on:  a forced FOUR or TWO_PLAIN (FIC: FOUR) runs vit_soft_lanes.hpp's soft four-lane / table-free two-lane decoder and is reported as such; a
 *        forced TWO (per-lane tables of hard metrics) still runs and reports LANE.  Under DABHIP_FORM_AUTO the knobs DABHIP_VIT_SOFT_FOUR_LANES and
 *        DABHIP_FIC_SOFT_FOUR_LANES (0 / 1 / N groups resp. tiles; defaults in decoder_form.hpp from profiles/r08_soft_lanes_curve.json: 1176 groups, 0 tiles) choose
 *        between FOUR and LANE.  Hard-decision engines are not affected.
 * dabhip_engine_set_soft_lanes may be called at any time; it only changes which kernel a later launch takes, never the bytes.
 * dabhip_engine_decoder_forms: bit f of *msc_mask / *fic_mask is set when form f ran in at least one launch since the last
 * dabhip_engine_decode or dabhip_stage_fic_decode began (0: no such launch, e.g. no MSC frame).  Either pointer may be NULL. */
#define DABHIP_FORM_AUTO (-1)
#define DABHIP_FORM_WAVE 0
#define DABHIP_FORM_LANE 1
#define DABHIP_FORM_TWO 2
#define DABHIP_FORM_TWO_PLAIN 3
#define DABHIP_FORM_FOUR 4
int dabhip_engine_set_decoder_forms(dabhip_engine *e, int msc_form, int fic_form);
int dabhip_engine_set_soft_lanes(dabhip_engine *e, int enable);
int dabhip_engine_decoder_forms(const dabhip_engine *e, uint32_t *msc_mask, uint32_t *fic_mask);

/* Parity guard (default ON).  The reference takes its hard decisions as sign tests on fp64 FFTW spectra (input_sdr.c:132-162);
 * the OFDM stage here transforms in fp32.  With the guard on, every decision whose |Re| or |Im| of cur*conj(prev) lies inside
 * the fp32 error band is re-decided in fp64 from the int8 samples, so the demapped bits -- and therefore the ETI bytes -- are
 * those exact arithmetic gives.  `level`:
 *   DABHIP_GUARD_OFF (0)       raw fp32 decisions; their disagreement rate is what dabhip_stage_decision_audit measures;
 *   DABHIP_GUARD_MEASURED (1)  the band is >= 4.5 x the worst error measured over > 10^10 audited decisions ("exact with measured margin");
 *   DABHIP_GUARD_PROVEN (2)    the band is a rigorous forward-error bound of this very transform and product ("exact by construction":
 *                              DESIGN.md section 3 carries the derivation, tools/fft_error_bound.py the arithmetic); 13 x as wide, i.e. 13 x
 *                              the re-decisions on noisy input, none on clean input;
 *   DABHIP_GUARD_DEFAULT (-1)  the library's default level (dabhip_parity_guard_default_level()).
 * Applies to hard decisions without the software AFC (the two configurations that claim reference semantics). */
#define DABHIP_GUARD_DEFAULT (-1)
#define DABHIP_GUARD_OFF 0
#define DABHIP_GUARD_MEASURED 1
#define DABHIP_GUARD_PROVEN 2
int dabhip_engine_set_parity_guard(dabhip_engine *e, int level);
int dabhip_engine_parity_guard_level(const dabhip_engine *e);
int dabhip_parity_guard_default_level(void);
/* the two constants of a level: bound on a bin's error relative to sqrt(sum |x_n|^2), bound on the product's rounding relative to |cur|_1 |prev|_1 */
int dabhip_parity_guard_constants(int level, double *bin_c, double *prod_c);
/* The proven level lists per bin: raw bin k's error bound is this fraction (0.33 .. 1) of the level's bin constant -- the bound's stage terms depend on the
 * bin's index digits; < 0: no such bin. */
double dabhip_parity_guard_bin_scale(int raw_bin);
/* Decisions the guard re-decided in the last decode, and hard decisions taken in all. */
int dabhip_engine_guard_stats(const dabhip_engine *e, int64_t *flagged, int64_t *decisions);
/* The guard lists the decisions to re-decide per kernel launch (64 entries per TF, at least 262,144; the proven level: 1024, 1,048,576).  A launch with more of them
 * -- input that synchronises but has many near-zero products: strongly notched, narrowband or near-DC frames -- does not fail: its
 * frames are decided again in full from fp64 transforms (slow, still the bits of exact arithmetic).  Number of such launches in the
 * last decode; and the list capacity as a test knob (0 = automatic). */
int dabhip_engine_guard_overflows(const dabhip_engine *e);
int dabhip_engine_set_guard_list_cap(dabhip_engine *e, uint32_t cap);

/* Launch limits (test knob, per engine).  A decode larger than one launch can hold is split: the MSC decoder into slices by survivor-record rows, the
 * regroup and the FIC group by tiles of 64 records, a session's device gather by descriptors, the two-kernel OFDM stage into chunks of transmission frames
 * (its FIC pre-pass: 19 x as many); and scan results of more than a number of 32-bit words come back by copy-engine commands instead of one kernel.  No
 * test-sized input reaches the defaults, so the limits can be lowered: limits[0 .. DABHIP_LAUNCH_LIMITS) in the order of the DABHIP_LIMIT_* indices, 0 = the
 * default (48 << 20 rows, 32768 tiles, 32768 tiles, 65535 descriptors, 1 << 18 words, 4096 frames).  The output does not depend on them.  Refused (-1, the
 * limits stay as they were): a negative value, a regroup limit that is not a multiple of 8 or above 32768, a FIC-group or device-gather limit above 65535,
 * an OFDM chunk above 1 << 20.
 * dabhip_*_launch_report: what the last decode / segment / stage entry / process_frame did -- out[DABHIP_REPORT_*], at most cap values; returns their number.
 * DABHIP_REPORT_FETCH_FORM: 0 = no scan ran, 1 = one kernel, 2 = copy-engine commands.  A session counts the device gathers since the previous feed returned.
 * The counts are launches MADE: when a stream breaks the split scan's assumption and is scanned again, the frames are laid out and stage A runs a second
 * time, so DABHIP_REPORT_FIC_PREPASS (two-kernel stage) is twice the pieces of the final frame list and DABHIP_REPORT_FETCHES is 2; dabhip_engine_demapped_tf
 * completing deferred frames adds its launches to DABHIP_REPORT_OFDM_CHUNKS.  DABHIP_REPORT_DECODER_PLANNED: the slices the host's plan of the MSC batch
 * holds; DABHIP_REPORT_DECODER (launches made) equals it. */
#define DABHIP_LAUNCH_LIMITS 6
#define DABHIP_LIMIT_DECISION_ROWS 0
#define DABHIP_LIMIT_REGROUP_TILES 1
#define DABHIP_LIMIT_FIC_GROUP_TILES 2
#define DABHIP_LIMIT_GATHER_DESCS 3
#define DABHIP_LIMIT_FETCH_WORDS 4
#define DABHIP_LIMIT_FFT_CHUNK_TFS 5
#define DABHIP_REPORT_VALUES 10
#define DABHIP_REPORT_DECODER 0
#define DABHIP_REPORT_REGROUP 1
#define DABHIP_REPORT_FIC_GROUP 2
#define DABHIP_REPORT_GATHER 3
#define DABHIP_REPORT_OFDM_CHUNKS 4
#define DABHIP_REPORT_FIC_PREPASS 5
#define DABHIP_REPORT_FETCH_FORM 6
#define DABHIP_REPORT_FETCHES 7
#define DABHIP_REPORT_GATHER_CALLS 8
#define DABHIP_REPORT_DECODER_PLANNED 9
int dabhip_engine_set_launch_limits(dabhip_engine *e, const int64_t *limits, int n);
int dabhip_engine_launch_report(const dabhip_engine *e, int64_t *out, int cap);
/* The MSC batch of the last decode as the host planned it: the trellis steps of every wave-group of 64 code words in launch order (nsteps, at most cap
 * values; a group takes ceil(steps / 8) * 8 survivor-record rows) and the tiles of 64 records the regroup covers.  Returns the number of groups. */
int dabhip_engine_msc_plan(const dabhip_engine *e, int32_t *nsteps, int cap, int64_t *ntiles);
/* sizeof the front end's per-stream state: a scan fetches nstreams * max_calls * 2 + nstreams + 1 + nstreams * this / 4 words at most */
int dabhip_host_stream_state_bytes(void);

/* Sub-channel filter (the reference's TODO.md:28-31, "save CPU time by not decoding data which will later be discarded"):
 * only the listed SubChIds (0..63) are decoded and carried; the ETI frames then list exactly those in their STC (NST, FL,
 * HCRC and EOF CRC follow; the FIC is passed on unchanged), each one's payload identical to the unfiltered frame's.
 * n <= 0 = all (default, the reference's frames).  Takes effect with the next decode.
 * Ids outside 0..63 are ignored, and so is a repeated id; a list with no valid id (n > 0) carries nothing: every frame has NST 0 and the FIC alone, and
 * no MSC code word is decoded.  A listed id the ensemble does not signal (yet) is simply absent from the STC until it is.
 * The fault flags of dabhip_engine_stream_status describe the carried multiplex (see there); lock, the CIF counter and the operator log
 * (dabhip_engine_stream_log: it dumps the whole ensemble) do not depend on the filter. */
int dabhip_engine_set_subchannels(dabhip_engine *e, const int32_t *ids, int n);

/* OFDM stage variant.  enable != 0 (default): the 2048-point transforms and the DQPSK demap / de-interleave scatter run as
 * ONE kernel that never writes the complex64 spectra (311,296 B read + 28,800 B written per TF).  enable == 0: the two
 * kernels K2 (cu8 -> complex64 spectra, 1,556,480 B per TF: the HBM-roofline stage of SURVEY.md 8(d)) and K2b (spectra ->
 * bits, re-reading the 1.2 MB).  Output bits -- and soft values -- hence ETI bytes, are identical in both.
 * dabhip_engine_fft_stats describes whichever kernel ran; dabhip_engine_fft_roofline measures K2 by itself. */
int dabhip_engine_set_fused(dabhip_engine *e, int enable);

/* Lock-in skip.  The reference's back end takes MSC data only from transmission frames it is locked on (dab_process_frame, dab.c:46-98: lock needs
 * ten consecutive TFs with 12 of 12 good FIBs, the 16-CIF ring starts with the TF that reaches lock, a loss drops it).  So of a stream that is not
 * locked when a decode (or a session's segment) starts, the first 9 - okcount TFs cannot be locked whatever their FIBs say
 * (dabhip_host_lockin_deferred), and the OFDM stage demodulates only their FIC symbols: no ETI frame reads their MSC symbols.  A stream that is
 * locked at the start of a segment is demodulated in full.  ETI bytes are identical either way.
 * on != 0 (or the environment variable DABHIP_DEMOD_ALL=1): every TF is demodulated in full.  Default: off.
 * dabhip_engine_msc_deferred: TFs of the last decode whose MSC symbols were deferred (dabhip_engine_demapped_tf completes them on demand). */
int dabhip_engine_set_demod_all(dabhip_engine *e, int on);
int dabhip_engine_msc_deferred(const dabhip_engine *e);

/* Schedule of K1's per-stream chain (sdr_demod's FIFO + time synchronisation, input_sdr.c:36-84, where call n + 1 is positioned by what call n
 * found).  mode 0: the chain, call after call.  mode 1: with a look-ahead pass -- what a call computes from its frame (null-symbol energy,
 * fine time search) depends only on where in the stream its read began, and a locked receiver's reads begin within a few samples of a predictable
 * place: one pass computes both for every remaining call and every start position near the predicted one, all at once, and the chain looks them up
 * (and computes them itself where a read began elsewhere).  Same results in every case, call for call.  mode -1 (default): the pass for small
 * batches (where the chain leaves most of the device idle), the plain chain for large ones; DABHIP_K1_SPEC in the environment sets the default.
 * Mode 1 is a test / measurement knob: it is honoured up to 512 streams (beyond that the pass cannot help and its table would run to tens of megabytes).
 * dabhip_engine_stage_ms reports the calls served from the pass's table as "sync_spec_calls". */
int dabhip_engine_set_sync_speculation(dabhip_engine *e, int mode);

/* ---- several devices of one node (BASELINE configs[3]: 2048 streams = 256 per GPU x 8) --------------
 * dab2eti.c:237,279-302 drives ONE device from one demod thread.  A batch of independent ensembles shards by stream with no
 * data exchange at all: the streams of a decode are dealt to the listed devices in contiguous slices (slice i of n takes B / n
 * streams, the first B mod n slices one more: 2048 on 8 = stream s on device s / 256; 10 on 4 = 3, 3, 2, 2 -- dabhip_multi_plan
 * answers for any batch size, before the decode), every slice is a complete batch engine with its own persistent host thread and HIP streams, and all slices decode at
 * once.  No collective, no peer access.  Frames are read back per GLOBAL stream index, or drained in stream order.
 * A device may be listed more than once (each entry is its own slice).  iq[b]: host pointers, or -- on_device != 0 --
 * device pointers that live on the device of stream b's slice (dabhip_multi_slice_of). */
typedef struct dabhip_multi dabhip_multi;
dabhip_multi *dabhip_multi_create(const int *devices, int n);
void dabhip_multi_destroy(dabhip_multi *m);
int dabhip_multi_slices(const dabhip_multi *m);
/* Slice and device that decode `stream` of a batch of `nstreams` -- the dealing rule itself, valid before the first decode (device pointers of
 * an on_device decode must live on that device).  0, <0 on error. */
int dabhip_multi_plan(const dabhip_multi *m, int nstreams, int stream, int *slice, int *device);
/* The same for the size of the LAST dabhip_multi_decode (-1 before the first one). */
int dabhip_multi_slice_of(const dabhip_multi *m, int stream, int *device);
/* Host placement of a slice (dab2eti.c:237 is the one unplaced demod thread this replaces): its decode thread, control-plane pool and host lane are
 * bound to a chunk of the CPUs of its device's NUMA node (/sys/bus/pci/devices/<bdf>/numa_node; the slices of a node get disjoint chunks), and its
 * page-locked buffers are allocated by those threads.  Returns the number of CPUs (0 = unbound: single-socket machine, node unknown, DABHIP_NUMA=0)
 * and writes up to cap of them. */
int dabhip_multi_slice_cpus(const dabhip_multi *m, int slice, int32_t *cpus, int cap, int *numa_node);
int64_t dabhip_multi_decode(dabhip_multi *m, const uint8_t *const *iq, const size_t *nbytes, int nstreams, int on_device);
int64_t dabhip_multi_eti_count(const dabhip_multi *m, int stream);
uint32_t dabhip_multi_stream_status(const dabhip_multi *m, int stream);   /* as dabhip_engine_stream_status, global stream index */
int64_t dabhip_multi_eti_read(dabhip_multi *m, int stream, uint8_t *dst, int64_t cap_frames);
int64_t dabhip_multi_stream_log(dabhip_multi *m, int stream, char *buf, int64_t cap);   /* as dabhip_engine_stream_log, global stream index */
int64_t dabhip_multi_eti_drain(dabhip_multi *m, dabhip_eti_sink sink, void *user);   /* all frames, global stream order */
int dabhip_multi_trace(const dabhip_multi *m, int stream, int32_t *ints6, double *ffs, int cap_calls);
/* The engine of one slice, for the per-engine queries (stage times, guard statistics); owned by the multi object. */
dabhip_engine *dabhip_multi_engine(dabhip_multi *m, int slice);
/* Wall clock (ms) of the last decode: the whole call (slice < 0) or one slice's own decode on its host thread. */
float dabhip_multi_wall_ms(const dabhip_multi *m, int slice);
int dabhip_multi_set_afc(dabhip_multi *m, int enable);
int dabhip_multi_set_soft(dabhip_multi *m, int enable);
int dabhip_multi_set_soft_lanes(dabhip_multi *m, int enable);   /* dabhip_engine_set_soft_lanes on every device */
int dabhip_multi_set_parity_guard(dabhip_multi *m, int level);
int dabhip_multi_set_fused(dabhip_multi *m, int enable);
int dabhip_multi_set_subchannels(dabhip_multi *m, const int32_t *ids, int n);

/* ---- streaming sessions ---------------------------------------------
 * The batch engine over UNBOUNDED streams: B parallel captures fed segment by segment (stdin, a socket, a file too
 * large for the device).  The state dab2eti keeps between calls -- FIFO backlog and stale frame tail (sdr_fifo.c),
 * timing corrections (input_sdr.c:36-112), lock counter and the 16-CIF ring (dab.c:35-98) -- is carried on the device and
 * in the host control plane, so the ETI frames of all segments, concatenated, are byte-identical to one
 * dabhip_engine_decode() of the whole capture, whatever the segment sizes (they need not be multiples of 262144).
 * After each feed the frames of THAT segment are read with the eti_* calls below. */
typedef struct dabhip_stream dabhip_stream;
dabhip_stream *dabhip_stream_create(int device, int nstreams);
/* the same with the host side chosen by the caller: host_threads of the control-plane pool (0 = automatic), CPUs to bind them to (ncpus = 0: unbound) */
dabhip_stream *dabhip_stream_create_on_cpus(int device, int nstreams, int host_threads, const int32_t *cpus, int ncpus);
void dabhip_stream_destroy(dabhip_stream *s);
/* Append nbytes[b] bytes to stream b (host pointers, or device pointers when on_device != 0) and decode every
 * 262144-byte call that became complete.  Returns the ETI frames produced by this segment, <0 on error. */
int64_t dabhip_stream_feed(dabhip_stream *s, const uint8_t *const *iq, const size_t *nbytes, int on_device);
/* Overlap of upload and decode: hand over the segment AFTER the one about to be fed.  Its upload starts at once on a stream
 * of its own and runs while dabhip_stream_feed decodes the segment before it; a later dabhip_stream_feed with the SAME
 * pointers and sizes consumes it.  Order of calls: prefetch(0) feed(0)  -or-  feed(0); then prefetch(k+1) feed(k) ...; at most
 * two segments may be waiting.  Host segments must be page-locked (dabhip_host_alloc) for the copy to run asynchronously and must
 * stay untouched until the feed that consumes them has returned.  Returns 0, <0 on error. */
int dabhip_stream_prefetch(dabhip_stream *s, const uint8_t *const *iq, const size_t *nbytes, int on_device);
/* The same session over streams that LIVE in device memory, read in place (no copy into windows): base[b][x] (device memory) is byte x of stream b
 * counted from the session's start, avail[b] the bytes that are there now (it only grows).  The caller keeps the bytes from
 * dabhip_stream_need_from(s, b) on where they are -- a linear buffer that is appended to -- and may recycle everything below.  Not to be mixed
 * with dabhip_stream_feed / _prefetch on one session.  Returns the ETI frames produced by the new bytes, <0 on error. */
int64_t dabhip_stream_feed_resident(dabhip_stream *s, const uint8_t *const *base, const size_t *avail);
int64_t dabhip_stream_need_from(const dabhip_stream *s, int stream);   /* oldest stream byte a later segment may still read; <0: bad argument */
int64_t dabhip_stream_eti_count(const dabhip_stream *s, int stream);
int dabhip_stream_stage_ms(const dabhip_stream *s, const char **names, float *ms, int cap);   /* of the segment fed last; names as dabhip_engine_stage_ms */
uint32_t dabhip_stream_status(const dabhip_stream *s, int stream);        /* as dabhip_engine_stream_status, sticky over the session's segments */
int64_t dabhip_stream_log(dabhip_stream *s, int stream, char *buf, int64_t cap);   /* as dabhip_engine_stream_log: the operator messages since the last call */
int64_t dabhip_stream_eti_read(dabhip_stream *s, int stream, uint8_t *dst, int64_t cap_frames);
int64_t dabhip_stream_eti_drain(dabhip_stream *s, dabhip_eti_sink sink, void *user);
/* as dabhip_engine_eti_fetch / _wait, for the frames of the segment fed last: its download overlaps the next segment's upload and decode */
int64_t dabhip_stream_eti_fetch(dabhip_stream *s, uint8_t *dst, int64_t cap_frames);
int dabhip_stream_eti_fetch_wait(dabhip_stream *s);
int dabhip_stream_set_afc(dabhip_stream *s, int enable);
int dabhip_stream_set_subchannels(dabhip_stream *s, const int32_t *ids, int n);   /* before the first segment only */
int dabhip_stream_set_soft(dabhip_stream *s, int enable);   /* before the first segment only */
int dabhip_stream_set_soft_lanes(dabhip_stream *s, int enable);   /* dabhip_engine_set_soft_lanes for the session; any time */
int dabhip_stream_set_parity_guard(dabhip_stream *s, int level);   /* see dabhip_engine_set_parity_guard */
int dabhip_stream_set_sync_speculation(dabhip_stream *s, int mode);   /* default -1, see dabhip_engine_set_sync_speculation */
int dabhip_stream_set_demod_all(dabhip_stream *s, int on);            /* see dabhip_engine_set_demod_all */
int dabhip_stream_msc_deferred(const dabhip_stream *s);               /* TFs of the segment fed last whose MSC symbols were deferred */
/* launch limits and the launches of the segment fed last (single-device sessions): see dabhip_engine_set_launch_limits */
int dabhip_stream_set_launch_limits(dabhip_stream *s, const int64_t *limits, int n);
int dabhip_stream_launch_report(const dabhip_stream *s, int64_t *out, int cap);
/* ---- sessions over several devices of one node -----------------------------------------------------------------------
 * dab2eti.c:60-130,237 is a session on ONE device: calls arrive for ever from one demod thread.  B independent unbounded streams shard like a batch
 * does: the streams are dealt ONCE, at creation, to the listed devices in contiguous slices (the rule of dabhip_multi_plan: slice i of n takes
 * B / n streams, the first B mod n slices one more), every slice is a complete dabhip_stream session on its device with its own host thread, and
 * every call below is that call made on all slices at once with each slice's part of the pointer arrays.  No collective, no peer access.  The
 * frames of a segment are byte-identical to those of ONE dabhip_stream session over all B streams (and, concatenated over the segments, to one
 * dabhip_engine_decode of the whole captures), in global stream order.  A device may be listed more than once (each entry is its own slice).
 * iq[b] / base[b]: host pointers (page-locked for asynchronous uploads: dabhip_host_alloc memory is visible to every device), or -- on_device /
 * feed_resident -- device pointers that live on the device of stream b's slice (dabhip_multi_stream_slice_of).
 * Call sequence of a host-fed pipeline (what `dab2eti-hip --stream --devices 0-7` does):
 *     prefetch(seg 0); loop k: prefetch(seg k + 1); n = feed(seg k); eti_fetch(out[k & 1], n); ... a writer thread: eti_fetch_wait(); write(out[k & 1]). */
typedef struct dabhip_multi_stream dabhip_multi_stream;
dabhip_multi_stream *dabhip_multi_stream_create(const int *devices, int n, int nstreams);
void dabhip_multi_stream_destroy(dabhip_multi_stream *m);
int dabhip_multi_stream_slices(const dabhip_multi_stream *m);
int dabhip_multi_stream_streams(const dabhip_multi_stream *m);
/* slice index of `stream` (< 0: bad argument); its device, and the slice's first stream and stream count */
int dabhip_multi_stream_slice_of(const dabhip_multi_stream *m, int stream, int *device, int *first, int *count);
/* one slice's session, for the per-session queries (dabhip_stream_stage_ms); owned by the multi object, NULL for an empty slice */
dabhip_stream *dabhip_multi_stream_session(dabhip_multi_stream *m, int slice);
int dabhip_multi_stream_prefetch(dabhip_multi_stream *m, const uint8_t *const *iq, const size_t *nbytes, int on_device);
int64_t dabhip_multi_stream_feed(dabhip_multi_stream *m, const uint8_t *const *iq, const size_t *nbytes, int on_device);
int64_t dabhip_multi_stream_feed_resident(dabhip_multi_stream *m, const uint8_t *const *base, const size_t *avail);
int64_t dabhip_multi_stream_need_from(const dabhip_multi_stream *m, int stream);
int64_t dabhip_multi_stream_eti_count(const dabhip_multi_stream *m, int stream);
uint32_t dabhip_multi_stream_status_of(const dabhip_multi_stream *m, int stream);   /* as dabhip_stream_status, global stream index (dabhip_multi_stream_status is the batch object's) */
int64_t dabhip_multi_stream_eti_read(dabhip_multi_stream *m, int stream, uint8_t *dst, int64_t cap_frames);
int64_t dabhip_multi_stream_log_of(dabhip_multi_stream *m, int stream, char *buf, int64_t cap);   /* as dabhip_stream_log, global stream index */
int64_t dabhip_multi_stream_eti_drain(dabhip_multi_stream *m, dabhip_eti_sink sink, void *user);   /* frames of the segment fed last, global stream order */
/* all frames of the segment fed last in global stream order, one asynchronous download per slice into dst (page-locked); _wait: they have landed */
int64_t dabhip_multi_stream_eti_fetch(dabhip_multi_stream *m, uint8_t *dst, int64_t cap_frames);
int dabhip_multi_stream_eti_fetch_wait(dabhip_multi_stream *m);
int dabhip_multi_stream_set_afc(dabhip_multi_stream *m, int enable);
int dabhip_multi_stream_set_soft(dabhip_multi_stream *m, int enable);                    /* before the first segment only */
int dabhip_multi_stream_set_soft_lanes(dabhip_multi_stream *m, int enable);              /* any time */
int dabhip_multi_stream_set_parity_guard(dabhip_multi_stream *m, int level);
int dabhip_multi_stream_set_sync_speculation(dabhip_multi_stream *m, int mode);
int dabhip_multi_stream_set_subchannels(dabhip_multi_stream *m, const int32_t *ids, int n);   /* before the first segment only */

/* Page-locked host memory for segments: fill the next one while the current one decodes (double buffering). */
void *dabhip_host_alloc(size_t nbytes);
void dabhip_host_free(void *p);

/* Streaming rates of the device, for reading the K2 roofline figure against what a bare kernel reaches (not on the data path):
 * gbs[0] fill, gbs[1] copy, gbs[2] K2's mix (1 byte read per 4 written), GB/s of bytes moved, over buffers of `bytes` bytes. */
int dabhip_stream_ceiling(int device, size_t bytes, int reps, double *gbs);

/* Which physical device an index is: its PCI bus id ("0000:c1:00.0", cap_bus >= 16) and name.  bench.py records both per rank and refuses to report
 * a multi-rank figure whose ranks did not sit on distinct devices.  0, <0: no such device. */
int dabhip_device_identity(int device, char *bus_id, int cap_bus, char *name, int cap_name);

/* Device memory for callers without a GPU runtime of their own: the batch entries (dabhip_engine_decode with on_device,
 * dabhip_synth_generate_device, the stage entries) take plain device pointers.  copy: to_device != 0: host -> device. */
void *dabhip_device_alloc(size_t nbytes, int device);
void dabhip_device_free(void *p);
int dabhip_device_copy(void *dst, const void *src, size_t nbytes, int to_device);

/* What the OFDM stage of the LAST dabhip_engine_decode left for transmission frame `tf` (0-based among the frames `stream`
 * demodulated in that decode) -- the content of tf->fic_symbols_demapped[3][3072] and tf->msc_symbols_demapped[72][3072]
 * (dab.h:27-33, filled at input_sdr.c:146-162) as the batch path holds it: 9216 + 221184 values, 0 / 1 for hard decisions, the
 * signed 4-bit values (-7 .. 7) with soft decisions on.  Host arrays.  0, <0 on error.
 * A TF whose MSC symbols the decode deferred (lock-in skip, dabhip_engine_set_demod_all) is completed on demand: the first such request runs the MSC
 * symbols of ALL deferred TFs of that decode through the configured OFDM stage, from that decode's samples -- host input lives on in the engine's
 * own upload buffer; with dabhip_engine_decode_device the caller's buffers must still be in place and unchanged.  (The engine behind a session
 * cannot complete a deferred TF it carried over from an earlier segment, whose samples may be gone: that request is an error.) */
int dabhip_engine_demapped_tf(dabhip_engine *e, int stream, int tf, int8_t *fic, int8_t *msc);

/* Per sdr_demod call trace of one stream, for parity with the reference's state after each
 * call: {ok, frame_read, coarse_timeshift, fine_timeshift, coarse_freq_shift, fifo_count}
 * as int32[6] per call plus fine_freq_shift as double per call. */
int dabhip_engine_trace(const dabhip_engine *e, int stream, int32_t *ints6, double *ffs, int cap_calls);
/* With the software AFC on: the re-tuning (Hz, relative to nominal) in effect during each call -- sdr->frequency of dab2eti.c:76-103 as the NCO
 * applied it to that call's samples; 0 everywhere in parity mode. */
int dabhip_engine_trace_nco(const dabhip_engine *e, int stream, int32_t *nco_hz, int cap_calls);

/* Timing of the stages of the last decode (milliseconds, HIP events on the engine's stream).
 * names: "sync", "fft", "demap", "fic", "control", "gather", "viterbi", "eti", then host wall-clock
 * phases "host_setup", "host_frames", "host_worklist" and the total "wall"; then, for a host-fed decode (on_device == 0),
 * "h2d" (ms of the IQ upload, HIP events), "h2d_mbytes" (10^6 bytes uploaded) and "h2d_pinned_mbytes" (how much of that came
 * straight from page-locked memory; the rest went through the engine's staging ring); and "sync_fp64_calls": calls whose coarse
 * frequency arg-max the single-precision first pass of K1's verification left to the fp64 pass (a count, not a time); "sync_spec_calls": calls of
 * K1's chain whose estimators came out of the look-ahead pass's table (dabhip_engine_set_sync_speculation; 0 when the plain chain ran).
 * Returns number of entries written. */
int dabhip_engine_stage_ms(const dabhip_engine *e, const char **names, float *ms, int cap);
/* Per-launch statistics of the OFDM FFT kernel in the last decode: number of launches,
 * transmission frames transformed, total kernel milliseconds (HIP events). */
int dabhip_engine_fft_stats(const dabhip_engine *e, int64_t *launches, int64_t *tfs, double *ms);
/* K2 (ofdm_fft_kernel) alone, `reps` times over the transmission frames of the LAST decode: same resident IQ, same frame
 * list, same launch shape as the two-kernel stage (one untimed pass first).  HIP events on the engine's stream around
 * every launch: number of timed launches, TFs transformed, total kernel milliseconds.  This is the roofline
 * measurement for input_sdr.c:115-130 whichever OFDM variant the decode itself used. */
int dabhip_engine_fft_roofline(dabhip_engine *e, int reps, int64_t *launches, int64_t *tfs, double *ms);

/* ---- stage entries (parity tests) ------------------------------------------------------ */
/* OFDM FFT stage alone (replaces input_sdr.c:115-130): nframes contiguous cu8 frames of
 * 393216 bytes each (device pointers when on_device) -> fftshifted complex64 spectra
 * [nframes][76][2048][2].  `reps` > 1 repeats the launch for timing; kernel_ms (optional)
 * receives the mean duration of one launch from HIP events. */
int dabhip_stage_ofdm_fft(dabhip_engine *e, const uint8_t *frames, int nframes, float *spectra, int on_device,
                          int reps, float *kernel_ms);
/* DQPSK + demap + frequency de-interleave (input_sdr.c:132-162): spectra of nframes ->
 * fic bytes [nframes][9216] and msc bytes [nframes][221184] (host pointers). */
int dabhip_stage_demap(dabhip_engine *e, const float *spectra, int nframes, uint8_t *fic, uint8_t *msc);
/* Audit of the fp32 OFDM stage against fp64 (test / calibration tool): nframes contiguous cu8 frames through K2 + K2b
 * (guard_on: with the parity guard), then fp64 transforms of every symbol on the GPU and a comparison of all 230,400
 * decisions per frame.  out8 = {decisions, disagreements with fp64, disagreements on carriers the guard rule does not flag,
 * decisions the rule flags, max |X32 - X64| / sqrt(sum |x|^2), max error of Re/Im(cur conj(prev)) / (|cur|_1 s(l-1) + |prev|_1 s(l)),
 * max residual product error / (|cur|_1 |prev|_1), entries the demapper listed}. */
int dabhip_stage_decision_audit(dabhip_engine *e, const uint8_t *frames, int nframes, int on_device, int guard_on, double *out8);
/* The same audit of the kernel the DEFAULT decode runs (round 5): ofdm_demap_kernel's guarded build, through a fourth build of the same source that also
 * stores the bins it holds and the products it decides on; frames laid out as a decode lays them out.  out10[0..8) as above (the errors are those of the
 * fused kernel's own bins and products, [7] = entries it listed); out10[8] = 1 when the shipping build, run on the same frames, left exactly the same bits
 * (guard_on = 0 only; -1 otherwise), out10[9] = 1 when it listed the same number of decisions. */
int dabhip_stage_decision_audit_fused(dabhip_engine *e, const uint8_t *frames, int nframes, int on_device, int guard_on, double *out10);
/* FIC decode of nframes TFs (fic.c:160-208): 9216 demapped bytes each -> 12x32 FIB bytes + 12 flags each. */
int dabhip_stage_fic_decode(dabhip_engine *e, const uint8_t *fic, int nframes, uint8_t *fibs, uint8_t *crc_ok);

/* ---- host-side control plane, callable without a GPU (used by the CPU test-suite) ------ */
/* FIG 0/0, 0/1, 0/2 parse of the 12 FIBs of one TF (fib_decode, fic.c:132-147).
 * hdr3 = {EId, CIFCount_hi, CIFCount_lo}; sub = 64 rows of
 * {id, slForm, uep_index, start_cu, size, bitrate, protlev, ASCTy}. */
int dabhip_host_parse_fibs(const uint8_t *fibs, const uint8_t *crc_ok, int32_t *hdr3, int32_t *sub);
/* The lock-in rule (dab.c:46-52): how many of the next ntf TFs of a stream cannot be locked, given the back end's state in front of them
 * (locked; okcount = consecutive TFs with 12 of 12 good FIBs so far): locked ? 0 : min(ntf, max(0, 9 - okcount)). */
int dabhip_host_lockin_deferred(int locked, int okcount, int ntf);
/* ETI(NI) header (init_eti, misc.c:153-213) from the same table layout; returns its length. */
int dabhip_host_eti_header(const int32_t *hdr3, const int32_t *sub, uint8_t *out, int cap);
/* Lock FSM + 16-CIF ring + header sequence (dab_process_frame, dab.c:35-98) over ntf TFs
 * given their decoded FIBs (ntf x 384 bytes) and CRC flags (ntf x 12).  For each ETI frame
 * it would emit, writes first_cif[i] (linear index of the oldest CIF) and the header bytes
 * (272-byte rows) + lengths.  Returns the number of ETI frames. */
int dabhip_host_control_replay(const uint8_t *fibs, const uint8_t *crc_ok, int ntf, int32_t *first_cif,
                               uint8_t *headers, int32_t *header_len, int cap_frames);
/* the operator messages (see dabhip_engine_stream_log) of the calling thread's last dabhip_host_control_replay */
int64_t dabhip_host_control_replay_log(char *buf, int64_t cap);

/* The placement rule by itself (no GPU, no sysfs): slice i sits on NUMA node slice_node[i] (< 0: unknown); node_cpulist[n] is node n's CPU list in
 * the kernel's notation ("0-63,128-191").  cpu_slice[c] = the slice CPU c is given to, -1 = none; the slices of a node get disjoint contiguous
 * chunks of its list.  Returns the number of slices that got CPUs. */
int dabhip_host_placement_plan(const int32_t *slice_node, int nslices, const char *const *node_cpulist, int nnodes, int32_t *cpu_slice, int ncpu);
/* What the host pools are sized from (round 5): returns min(CPUs in the process's affinity mask, CFS quota of its cgroup), at least 1 -- NOT the
 * machine's thread count, which says nothing inside a container (DABHIP_CPUS=n overrides it); the two inputs come back in *affinity_cpus and
 * *cfs_quota_cpus (0 = no quota).  No GPU call.  dab2eti.c:237 has one demod thread and no pool to size. */
int dabhip_host_cpu_budget(int *affinity_cpus, int *cfs_quota_cpus);

/* The constant tables the kernels are built from (dab_tables.hpp generates them from the ETSI rules), so that tests can
 * hold them against the reference's literal arrays: which = 0: the 64 UEP profiles of ueptable (dab_tables.c:16-81) as rows
 * {bitrate, size, protection level, L1..L4, PI1..PI4} (PI as in ETSI, 1..24; the reference stores PI - 1); 1: pvec
 * (dab_tables.c:102-127), 24 x 32 flags; 2: rev_freq_deint_tab (dab_tables.c:164), 1536 entries; 3: the phase reference
 * symbol (sdr_prstab.c) as quarter turns, 1536 entries.  Returns the number of values written, <0 on error. */
int dabhip_host_table(int which, int32_t *out, int cap);

/* The FIFO of sdr_demod (cbWrite / sdr_read_fifo, sdr_fifo.c:26-61; input_sdr.c:36-55) as the sync-scan kernel keeps it:
 * in closed form over the resident stream.  One call = one sdr_demod call that appends chunk_bytes (input_buffer_len; 262144 from librtlsdr),
 * entered with the timing corrections the previous processed frame left in sdr->coarse_timeshift / fine_timeshift.  Returns 0 = nothing read
 * (fewer than 1.5 TF queued), 1 = the first frame, read and discarded (input_sdr.c:51-55), 2 = a frame read for
 * processing; <0 = error.  What sdr->buffer (393216 bytes) holds afterwards comes back in two parts.  Its last 1536 bytes -- the most a
 * negative time shift leaves unread (sdr_sync.c:197-201, sdr_fifo.c:56-59) -- as BYTES in tail[1536] (needs stream: the bytes fed so far;
 * null = not tracked).  Everything below as a view: buffer positions [seg_end[i-1], seg_end[i]) hold stream bytes seg_src[i] + position
 * (seg_src < 0: the calloc'ed zero bytes); 12 entries each. */
typedef struct dabhip_fifo dabhip_fifo;
dabhip_fifo *dabhip_host_fifo_new(void);
void dabhip_host_fifo_free(dabhip_fifo *f);
int dabhip_host_fifo_call(dabhip_fifo *f, int32_t coarse_timeshift, int32_t fine_timeshift, int32_t chunk_bytes, const uint8_t *stream,
                          int32_t *nseg, int32_t *seg_end, int64_t *seg_src, int32_t *fifo_count, uint8_t *tail);

/* ncalls further calls of 262144 bytes for a FIFO that reads without any time shift, counters only: what K1's look-ahead pass (sync_ahead_kernel)
 * predicts the stream's read pointer with, in closed form (the counters repeat every three calls).  Equals ncalls x dabhip_host_fifo_call(f, 0, 0,
 * 262144, ...) in `fed` (bytes appended so far) and `consumed` (stream offset of the read pointer); the frame-buffer view is left as it was.
 * Refused (-1) while a shift is pending or the first frame has not been dropped yet. */
int dabhip_host_fifo_skip_unshifted(dabhip_fifo *f, int32_t ncalls, int64_t *fed, int64_t *consumed);

/* ---- DAB+ audio (ETSI TS 102 563) ------------------------------------------------------- */
/* A stateful consumer of ETI frames that extracts the AUs of DAB+ sub-channels on the GPU: superframe sync on the fire code, RS(120,110)
 * correction of the s interleaved codewords of every superframe, AU CRCs.  Frames are pushed stream by stream; between pushes it keeps the last
 * 4 frames of every stream and the sync state of every (stream, sub-channel), so batches, sessions' fetched frames and a pipe all go through it.
 *
 * Sync rule, per (stream, sub-channel), walking the frames in order: unsynced, frame f starts a superframe if the raw (uncorrected) fire code
 * of its first 11 bytes passes and frames f..f+4 carry the sub-channel with the same STL (a multiple of 3 up to 216: 8 STL = 24 s bytes, s <= 72) and consecutive
 * FCTs (mod 250).  Synced, every 5th frame starts a candidate, whose frames must carry the locked STL with FCTs continuing the last
 * superframe's.  A gap or an STL change loses sync (the search restarts at that candidate's first frame); so does the 3rd consecutive candidate
 * whose raw fire code fails (the search restarts at the frame after it).  A candidate that loses sync is not decoded. */
typedef struct dabhip_dabplus dabhip_dabplus;
typedef struct dabhip_dabplus_sf {  /* one superframe of the last push */
  int32_t stream;
  int32_t sub;                      /* index into the SubChId list */
  int32_t fct;                      /* FCT of its first ETI frame */
  int32_t s;                        /* sub-channel rate / 8 kbit/s: 120 s bytes, 110 s of them audio */
  uint8_t fire_ok;                  /* fire code of the corrected bytes good */
  uint8_t layout_ok;                /* fire code good, au_start strictly increasing, every AU >= 3 bytes and inside 110 s */
  uint8_t rfa, dac_rate, sbr_flag, aac_channel_mode, ps_flag, mpeg_surround_config;
  int32_t num_aus;                  /* from (dac_rate, sbr_flag): 2, 3, 4 or 6 */
  uint16_t au_start[6];             /* AU offsets in the superframe (layout_ok only) */
  uint16_t au_len[6];               /* AU lengths including their 2 CRC bytes */
  uint32_t crc_ok;                  /* bit i: CRC of AU i good */
  int32_t rs_corrected;             /* bytes corrected by the RS decoder */
  int32_t rs_failed;                /* codewords beyond correction (left as received) */
} dabhip_dabplus_sf;
/* nsub SubChIds, the same for every stream.  NULL when there is no GPU (dabhip_last_error). */
dabhip_dabplus *dabhip_dabplus_create(int device, int nstreams, const int32_t *subch_ids, int nsub);
void dabhip_dabplus_destroy(dabhip_dabplus *d);
/* counts[s] ETI frames of stream s, stream after stream in `frames` (dabhip_engine_eti_device_ptr's layout): DEVICE memory when on_device != 0,
 * host memory otherwise (device frames need no alignment).  Returns the superframes completed by this call, <0 on error.
 * A frame carries a requested SubChId when its STC lists it, FICF set or not; if the STC lists the id more than once, the first entry counts
 * and the later ones are ignored, also when the first is no DAB+ sub-channel (STL 0, not a multiple of 3, above 216, or past byte 6144). */
int64_t dabhip_dabplus_push(dabhip_dabplus *d, const uint8_t *frames, const int64_t *counts, int on_device);
/* The superframes of the last push of one (stream, sub-channel index), in order: copies min(n, cap) records, returns n. */
int64_t dabhip_dabplus_superframes(const dabhip_dabplus *d, int stream, int sub, dabhip_dabplus_sf *out, int64_t cap);
/* Their corrected 110 s audio bytes, superframe after superframe (cap bytes at most); returns the byte count. */
int64_t dabhip_dabplus_data(const dabhip_dabplus *d, int stream, int sub, uint8_t *dst, int64_t cap);
/* Their AUs whose CRC is good, without the CRC bytes, one after another (boundaries: the records); returns the byte count. */
int64_t dabhip_dabplus_au_bytes(const dabhip_dabplus *d, int stream, int sub, uint8_t *dst, int64_t cap);
/* Counters since creation: superframes, fire-code fails, RS corrected bytes, RS failed codewords, AUs (of superframes with a good layout), AU
 * CRC fails, sync losses.  Returns 0, <0 on error. */
int dabhip_dabplus_stats(const dabhip_dabplus *d, int stream, int sub, int64_t *counters7);
/* GPU time of the last push in ms, stage by stage (names: "locate", "sync", "rs", "au", "carry"; as dabhip_engine_stage_ms); returns the count. */
int dabhip_dabplus_stage_ms(const dabhip_dabplus *d, const char **names, float *ms, int cap);

/* ---- packet-mode data (ETSI EN 300 401 clauses 5.3.2, 5.3.3, 5.3.5) ----------------------- */
/* A stateful consumer of ETI frames that extracts the packets of packet-mode sub-channels on the GPU, with the enhanced packet mode's outer
 * code RS(204,188) where a sub-channel is created with fec = 1.  Off unless asked for, and handled like dabhip_dabplus: frames are pushed
 * stream by stream, the state of every (stream, sub-channel) carries from push to push (at most 102 cells each), and any cutting of a stream
 * into pushes gives the same records.  These rules were written from the standard, not from a broadcast recording.
 *
 * Cells.  A sub-channel of 8 s kbit/s (STL = 3 s) carries s cells of 24 bytes per ETI frame; the cell stream of a (stream, SubChId) is the cells
 * of its frames in order.  A frame that lacks the id, or lists it with STL 0, an STL that is no multiple of 3 or a payload past byte 6144, breaks
 * the stream and gives no cells; a frame whose STL differs from the stream's breaks it and starts the next stream.  A break drops sync (counted as
 * a sync loss when there was sync) and every cell not consumed yet (counted as skipped).  If the STC lists the id twice, the first entry counts.
 *
 * Packet: 3 header bytes -- length code (2 bits: 1..4 cells), continuity index (2), first/last (2: 10 first, 00 intermediate, 01 last, 11 one and
 * only), address (10; 0 = padding), command (1), useful length (7; at most 24 L - 5) --, a data field of 24 L - 5 bytes with the useful bytes
 * first, and the CRC (x^16 + x^12 + x^5 + 1 from 0xFFFF, complemented, most significant byte first) over header and data field.
 *
 * FEC frame: 103 cells, 94 data cells (the 2256-byte application table) and 9 FEC cells of 2 header bytes (length code 00, a 4-bit counter 0..8,
 * address 1022) and 22 RS bytes: 192 parity bytes, then 6 zero bytes.  With Z the table followed by the parity, code word r (0..11) is Z[r + 12 c],
 * c = 0..203, byte c the coefficient of x^(203 - c); GF(256) by 0x11D, alpha = 2, generator prod (x + alpha^i), i = 0..15.  Decoding is bounded-
 * distance: a word within distance 8 of a code word is corrected, any other is left as received and counted as failed.
 *
 * FEC sync, per (stream, sub-channel) with fec = 1.  A run at cell k: cells k..k+8 carry the FEC header with counters 0..8.  Unsynced, the first
 * run at k makes sync; if the 94 cells before it are unconsumed cells of the unbroken stream, cells k-94..k+8 are a frame and are decoded, else
 * the unconsumed cells up to k+8 are skipped; the next frame starts at k+9.  Synced, every 103 cells are a frame: a hit when at least 5 of its 9
 * FEC cells carry their own header, which is RS-decoded; else a miss, which is walked as received and flagged.  The 3rd consecutive miss is not
 * walked: it loses sync, and the search resumes at the cell after that frame's first, with the frame's cells unconsumed.
 *
 * Walk.  The unit is the 94 data cells of an FEC frame after correction, or the s cells of one ETI frame without FEC.  From cell 0: the packet
 * that would start at cell k with length L is taken when k + L fits in the unit, its useful length is at most 24 L - 5 and its CRC is good,
 * then k += L; otherwise cell k is counted bad and k += 1.  Only taken packets give records (padding packets included). */
typedef struct dabhip_packet dabhip_packet;
#define DABHIP_PACKET_FROM_FEC 1    /* from an RS-decoded frame */
#define DABHIP_PACKET_FROM_MISS 2   /* from a missed frame, walked as received */
typedef struct dabhip_packet_rec {  /* one packet of the last push */
  int64_t cell;                     /* index of its first cell among the cells of its (stream, sub-channel) since creation */
  uint16_t address;
  uint8_t length;                   /* cells, 1..4 */
  uint8_t continuity;
  uint8_t first_last;               /* 2 first, 0 intermediate, 1 last, 3 one and only */
  uint8_t command;
  uint8_t useful_length;
  uint8_t flags;                    /* DABHIP_PACKET_FROM_* */
} dabhip_packet_rec;
/* nsub SubChIds with their FEC flags, the same for every stream.  NULL when there is no GPU (dabhip_last_error). */
dabhip_packet *dabhip_packet_create(int device, int nstreams, const int32_t *subch_ids, const uint8_t *fec_flags, int nsub);
void dabhip_packet_destroy(dabhip_packet *d);
/* counts[s] ETI frames of stream s, stream after stream in `frames`, in DEVICE memory when on_device != 0 (no alignment needed), else in host
 * memory.  Returns the packets taken by this call, <0 on error. */
int64_t dabhip_packet_push(dabhip_packet *d, const uint8_t *frames, const int64_t *counts, int on_device);
/* The packets of the last push of one (stream, sub-channel index), in order: copies min(n, cap) records, returns n. */
int64_t dabhip_packet_records(const dabhip_packet *d, int stream, int sub, dabhip_packet_rec *out, int64_t cap);
/* Their useful bytes, packet after packet (cap bytes at most); returns the byte count. */
int64_t dabhip_packet_data(const dabhip_packet *d, int stream, int sub, uint8_t *dst, int64_t cap);
/* Counters since creation: units walked (FEC frames, or ETI frames without FEC), missed frames walked, sync losses, cells skipped, bad cells,
 * packets, RS corrected bytes, RS failed code words.  Returns 0, <0 on error. */
int dabhip_packet_stats(const dabhip_packet *d, int stream, int sub, int64_t *counters8);
/* GPU time of the last push in ms, stage by stage (names: "locate", "sync", "gather", "rs", "cand", "walk", "carry"); returns the count. */
int dabhip_packet_stage_ms(const dabhip_packet *d, const char **names, float *ms, int cap);

/* Data groups out of the packets of ONE (stream, sub-channel), on the host.  Assembly runs per address != 0 over command = 0 packets.  A first or
 * only packet opens a group; an open group it finds unfinished is dropped and counted.  An intermediate or last packet is appended only to an
 * open group whose last packet's continuity index is one less (mod 4); with an open group and another index the group is dropped; with none it is
 * counted as an orphan.  A last or only packet completes the group.  A group that would pass 8208 bytes is dropped.  State carries from push to push. */
typedef struct dabhip_packet_groups dabhip_packet_groups;
typedef struct dabhip_packet_group {
  int32_t address;
  int32_t length;                   /* bytes, header and CRC included */
  uint8_t ext_flag, crc_flag, seg_flag, ua_flag;
  uint8_t type, continuity, repetition;
  uint8_t crc_ok;                   /* crc_flag set: the packet CRC-16 over all but the last two bytes equals them; else 0 */
  uint16_t ext_field;               /* ext_flag set */
  uint8_t last_segment;             /* seg_flag set */
  uint8_t header_ok;                /* the group is long enough for the header its flags announce (else the fields below are -1) */
  int32_t segment_number;           /* seg_flag set, else -1 */
  int32_t transport_id;             /* ua_flag and the transport id flag set, else -1 */
} dabhip_packet_group;
dabhip_packet_groups *dabhip_packet_groups_create(void);
void dabhip_packet_groups_destroy(dabhip_packet_groups *g);
/* nrecs records in order with their ndata useful bytes (dabhip_packet_records / _data).  Returns the groups this call completed, <0 on error. */
int64_t dabhip_packet_groups_push(dabhip_packet_groups *g, const dabhip_packet_rec *recs, int64_t nrecs, const uint8_t *data, int64_t ndata);
/* Group i of the last push: its record, and min(length, cap) of its bytes into dst (may be null); returns its length, <0 on error. */
int64_t dabhip_packet_groups_get(const dabhip_packet_groups *g, int64_t i, dabhip_packet_group *rec, uint8_t *dst, int64_t cap);
/* Counters since creation: groups completed, groups dropped, orphan packets, groups whose CRC failed.  Returns 0. */
int dabhip_packet_groups_stats(const dabhip_packet_groups *g, int64_t *counters4);

/* ---- MPEG-2 transport stream (ETSI TS 102 427; T-DMB video, TS 102 428, rides on it) ---------- */
/* A stateful consumer of ETI frames that extracts the MPEG-2 TS packets of stream-mode sub-channels on the GPU: slot sync on the 0x47 bytes,
 * the convolutional byte de-interleaver, RS(204,188).  Off unless asked for, and handled like dabhip_packet: frames are pushed stream by stream,
 * the state of every (stream, sub-channel) carries from push to push (at most 2447 bytes each), and any cutting of a stream into pushes gives
 * the same records.  These rules were written from the standard, not from a broadcast recording.
 *
 * Byte stream.  The byte stream of a (stream, SubChId) is the sub-channel's payload (8 STL bytes per ETI frame) of its frames, in order; if the
 * STC lists the id twice, the first entry counts.  A frame that lacks the id, or lists it with STL 0 or with a payload that runs past byte 6144,
 * breaks the stream and gives no bytes; a frame whose STL differs from the stream's breaks it and starts the next one.  A break drops sync
 * (counted as a sync loss when there was sync) and every byte not consumed yet (counted as skipped).  Positions count the bytes of the
 * (stream, sub-channel) since creation and go on counting across breaks.  Any STL is legal.
 *
 * Code word: 204 bytes, 188 TS bytes and then 16 parity bytes, byte k the coefficient of x^(203 - k); GF(256) by 0x11D, alpha = 2, generator
 * prod (x + alpha^i), i = 0..15 (the code of the enhanced packet mode above).  Decoding is bounded-distance: a word within distance 8 of a code
 * word is corrected, any other is left as received and flagged.
 *
 * Interleaver (I = 12, M = 17): byte k of a code word travels in branch k mod 12, delayed by 204 (k mod 12) bytes, so byte 0, the 0x47, is never
 * delayed.  If the slot of a code word starts at stream position P, its byte k lies at P + k + 204 (k mod 12); the word needs the 2448 bytes
 * P .. P + 2447.
 *
 * Sync, per (stream, sub-channel); `end` is the position one past the last byte on hand.  Unsynced, searching from q: with p the smallest
 * position >= q such that p + 816 < end and the five bytes at p + 204 i (i = 0..4) are all 0x47, bytes q .. p - 1 are skipped and the lane is
 * synced with its next slot at p and 0 misses; if there is none, the bytes below max(q, end - 816) are skipped and the search waits there for
 * the next push.  Synced with the next slot at P: if P + 2448 > end, wait (the bytes from P on carry to the next push).  Otherwise the slot is a
 * hit when the byte at P is 0x47 (the miss count becomes 0) and a miss when it is not (the count grows by 1).  On the 3rd consecutive miss sync is
 * lost and no packet is taken: one byte is skipped and the search resumes at P + 1 with the slot's other bytes unconsumed.  In every other case,
 * a second miss included, the word is gathered and RS-decoded and gives one record, flagged FROM_MISS on a miss; then P += 204. */
typedef struct dabhip_ts dabhip_ts;
#define DABHIP_TS_FROM_MISS 1       /* from a slot whose first byte was not 0x47 */
#define DABHIP_TS_RS_FAILED 2       /* no code word within distance 8: the bytes are as received */
#define DABHIP_TS_TEI 4             /* transport_error_indicator, as decoded */
#define DABHIP_TS_PUSI 8            /* payload_unit_start_indicator, as decoded */
#define DABHIP_TS_BAD_SYNC 16       /* byte 0 after decoding is not 0x47 */
typedef struct dabhip_ts_rec {      /* one packet of the last push */
  int64_t pos;                      /* position of its slot's first byte among the bytes of its (stream, sub-channel) since creation */
  uint16_t pid;
  uint8_t continuity;
  uint8_t flags;                    /* DABHIP_TS_* */
  uint8_t corrected;                /* bytes the RS decoder corrected, 0..8 */
  uint8_t pad[3];
} dabhip_ts_rec;
/* nsub SubChIds, the same for every stream.  NULL when there is no GPU (dabhip_last_error). */
dabhip_ts *dabhip_ts_create(int device, int nstreams, const int32_t *subch_ids, int nsub);
void dabhip_ts_destroy(dabhip_ts *d);
/* counts[s] ETI frames of stream s, stream after stream in `frames`, in DEVICE memory when on_device != 0 (no alignment needed), else in host
 * memory.  Returns the packets of this call, <0 on error. */
int64_t dabhip_ts_push(dabhip_ts *d, const uint8_t *frames, const int64_t *counts, int on_device);
/* The packets of the last push of one (stream, sub-channel index), in order: copies min(n, cap) records, returns n. */
int64_t dabhip_ts_records(const dabhip_ts *d, int stream, int sub, dabhip_ts_rec *out, int64_t cap);
/* Their 188 bytes each, packet after packet, failed words as received (whole packets, cap bytes at most); returns the byte count. */
int64_t dabhip_ts_data(const dabhip_ts *d, int stream, int sub, uint8_t *dst, int64_t cap);
/* Counters since creation: packets, packets from missed slots, sync losses, bytes skipped, RS corrected bytes, RS failed words, BAD_SYNC packets,
 * null packets (PID 0x1FFF).  Returns 0, <0 on error. */
int dabhip_ts_stats(const dabhip_ts *d, int stream, int sub, int64_t *counters8);
/* GPU time of the last push in ms, stage by stage (names: "locate", "runs", "sync", "jobs", "gather", "syndrome", "decode", "parse", "carry");
 * returns the count. */
int dabhip_ts_stage_ms(const dabhip_ts *d, const char **names, float *ms, int cap);

/* ---- ensemble directory (EN 300 401 clauses 5.2, 6, 8: the FIC's service information) ---------- */
/* A stateful consumer of ETI frames that reads the 96 FIC bytes of each on the GPU and keeps, per stream, what the ensemble carries: the
 * ensemble record, the sub-channels, the services with their components and labels, the packet-mode components.  Its answer names, for every
 * component, the sub-channel (and packet address, and FEC flag) that dabhip_dabplus, dabhip_packet and dabhip_ts ask their caller for.  Off
 * unless asked for and handled like dabhip_ts: frames are pushed stream by stream.  It is a strict parser of its own: the engine's control
 * plane keeps the reference's parse (control_plane.hpp), over-reads included.  These rules were written from the standard as remembered, not
 * from a copy of it nor from a broadcast recording; what this text, tests/dir_model.py, the modulator's si_mode and the
 * kernels agree on is what counts.
 *
 * Frames.  ETI(NI), 6144 bytes.  NST = byte 5 & 0x7F, FICF = byte 5 >> 7, MID = (byte 6 >> 3) & 3.  Every frame counts in `frames`.  FICF = 0:
 * the frame gives nothing and counts in `frames_without_fic`.  Else MID != 1 or NST > 64: nothing, `frames_skipped`.  Else the FIC is the 96
 * bytes at 12 + 4 NST: FIB 0, 1, 2 of 32 bytes, each counted in `fibs`.  The frames of a stream are numbered from 0 since creation (`frames`
 * before the frame); reset does not restart the numbers.
 *
 * FIB.  Bytes 30, 31 = ~CRC (high byte first), CRC-16-CCITT (x^16 + x^12 + x^5 + 1, initial value 0xFFFF, MSB first) of bytes 0..29.  A FIB
 * whose CRC fails counts in `fibs_crc_failed` and gives nothing else.
 *
 * FIG walk over bytes 0..29; nothing outside them is ever read.  i = 0.  While i < 30 and byte i != 0xFF: the FIG header is byte i, type =
 * top 3 bits, length = low 5 bits; `figs` += 1.  Length 0, or i + 1 + length > 30: `figs_truncated` += 1 and the walk of this FIB ends.  Else
 * the data field is the `length` bytes from i + 1, the FIG is taken as below, and i += 1 + length.  A FIG is exactly one of: handled, ignored
 * (`figs_ignored` += 1, no facts), or refused whole as truncated (type 1, 0/0, 0/9, 0/10).  Inside a handled FIG with a list of entries, the
 * entries are taken one after another from the body (the data field without its first byte); an entry that does not lie wholly inside the
 * body ends the FIG, `figs_truncated` += 1, earlier entries stand.  An empty body is legal and gives nothing.
 *
 * Type 0.  First data byte: C/N (bit 7), OE (6), P/D (5), extension (low 5).  OE = 1: ignored.  Else C/N = 1 and extension 1, 2, 3 or 14:
 * ignored.  Else by extension (every other one: ignored); multi-byte fields are big-endian:
 *   0/0   body >= 4 bytes, else truncated: EId(16); change flag(2) Al(1) CIF count high(5); CIF count low(8).  Further bytes are skipped.  One fact.
 *   0/1   entry: SubChId(6) start address(10); then the form bit (bit 7 of the third byte).  Short form, 3 bytes: form(1) table switch(1)
 *         UEP index(6); size, bit rate and protection level are the rows of ETSI table 7 (dab_tables.hpp: uep_table).  Long form, 4 bytes:
 *         form(1) option(3) level(2) size(10); protlev = level | option << 2, bit rate = size / m[protlev & 7] * (protlev & 4 ? 32 : 8)
 *         with m = 12, 8, 6, 4, 27, 21, 18, 15 (integer division; eep_size_multiple).  The table switch is not kept.  One fact per entry.
 *   0/2   entry: SId (16 bits if P/D = 0, 32 if P/D = 1); one byte local(1) CAId(3) number of components(4); then 2 bytes per component:
 *         TMId(2) and, TMId 0: ASCTy(6) SubChId(6) P/S(1) CA(1); TMId 1: DSCTy(6) SubChId(6) P/S CA; TMId 3: SCId(12) P/S CA; TMId 2: kept
 *         raw.  One fact per entry, with the whole component list.
 *   0/3   entry: SCId(12) rfa(3) SCCA flag(1); DG flag(1) rfu(1) DSCTy(6); SubChId(6) packet address(10); SCCA(16) only with the flag: 5 or 7
 *         bytes.  rfa and rfu are not kept; SCCA is kept as 0 without the flag.  One fact per entry.
 *   0/9   body >= 3 bytes, else truncated: the three bytes are kept raw (LTO byte, ECC, international table id); the rest is skipped.  One fact.
 *   0/10  body >= 4 bytes: rfu(1) MJD(17) LSI(1) rfa(1) UTC flag(1) hours(5) minutes(6); with the UTC flag, 2 more bytes: seconds(6)
 *         milliseconds(10), kept as 0 without.  A body shorter than 4, or 6 with the flag: truncated.  The rest is skipped.  One fact.
 *   0/14  every body byte is an entry: SubChId(6) FEC scheme(2).  One fact per byte.
 * Type 1.  First data byte: charset (high 4), OE (bit 3), extension (low 3).  OE = 1: ignored.  Extension 0: EId(16), 1: SId(16), 5: SId(32),
 * then 16 character bytes and a 16-bit character flag field: the data field must be exactly 21 bytes (0, 1) or 23 (5), else truncated.  One
 * fact: a label.  1/1 names the service (P/D 0, SId), 1/5 the service (P/D 1, SId).  Every other extension: ignored.
 * Types 2..7: ignored.
 * A FIB gives at most 28 facts (28 bytes of 0/14).  `facts` counts them.
 *
 * Directory, per stream since creation or the last reset: the ensemble record; 64 sub-channels indexed by SubChId; at most 64 services keyed
 * by (P/D, SId), each with its 0/2 byte, up to 15 raw two-byte component descriptors, and its label, charset and flag field; at most 64 packet
 * components keyed by SCId.  Facts are applied in the order (frame, FIB, byte offset).  An entry has one part per kind of fact that can reach
 * it: ensemble: 0/0, 0/9, 0/10, label (with the label's EId); sub-channel: 0/1, 0/14; service: 0/2, label; packet component: 0/3.  A fact
 * whose key exists replaces the part of its kind and no other (a 0/2 fact the whole component list; a label leaves the components alone and
 * the reverse).  A new key is appended, so services and packet components stand in order of first appearance.  A fact that needs a new key
 * in a full table is dropped and counts in `overflow_dropped`.  Every entry keeps first_frame and last_frame, the frame numbers of the first
 * and the latest fact applied to it, and `changes`: the facts that found their part present and altered a kept field of it (a first fact of
 * its kind is no change).  `facts_changed` counts the same over the stream.  The ensemble's time_frame is the frame of the latest 0/10.
 * A FIG never spans FIBs, so nothing is carried: any cutting of a stream into pushes gives the same directory.
 *
 * Complete: 0/0 and the ensemble label seen; at least one service; every service has its 0/2 part and its label; every TMId 0 or 1 component's
 * sub-channel has its 0/1 part; every TMId 3 component's SCId has a 0/3 entry whose sub-channel has its 0/1 part.
 *
 * Resolve (stream, P/D, SId, component index): kind MP2 (TMId 0, ASCTy 0), DABPLUS (TMId 0, ASCTy 63), TS (TMId 1, DSCTy 24), STREAM_DATA
 * (other TMId 1), PACKET (TMId 3), UNKNOWN (TMId 2: no sub-channel, subch = -1; other TMId 0); the SubChId; for PACKET the packet address, DG
 * flag, DSCTy and fec = (the sub-channel's 0/14 scheme == 1; 0 when no 0/14 was seen).  A missing link is an error, never a guess:
 * DABHIP_DIR_NO_SERVICE, _NO_COMPONENT (no 0/2 part, or the index past its list), _NO_PKTCOMP (no 0/3 for the SCId), _NO_SUBCH (no 0/1 for
 * the sub-channel). */
typedef struct dabhip_dir dabhip_dir;
enum { DABHIP_DIR_UNKNOWN = 0, DABHIP_DIR_MP2 = 1, DABHIP_DIR_DABPLUS = 2, DABHIP_DIR_TS = 3, DABHIP_DIR_STREAM_DATA = 4, DABHIP_DIR_PACKET = 5 };
enum { DABHIP_DIR_NO_SERVICE = -2, DABHIP_DIR_NO_COMPONENT = -3, DABHIP_DIR_NO_PKTCOMP = -4, DABHIP_DIR_NO_SUBCH = -5 };
#define DABHIP_DIR_HAVE_00 1        /* dabhip_dir_ensemble_rec.have */
#define DABHIP_DIR_HAVE_09 2
#define DABHIP_DIR_HAVE_10 4
#define DABHIP_DIR_HAVE_LABEL 8
#define DABHIP_DIR_SUB_HAVE_01 1    /* dabhip_dir_subch.have */
#define DABHIP_DIR_SUB_HAVE_14 2
#define DABHIP_DIR_SVC_HAVE_02 1    /* dabhip_dir_service.have */
#define DABHIP_DIR_SVC_HAVE_LABEL 2
typedef struct dabhip_dir_ensemble_rec {
  uint8_t have;                     /* DABHIP_DIR_HAVE_*; 0: nothing seen, the rest is zero */
  uint8_t charset;
  uint16_t eid;                     /* 0/0 */
  uint16_t label_eid;               /* 1/0 */
  uint16_t char_flags;
  uint8_t label[16];
  uint8_t change_flag, al, cif_hi, cif_lo;
  uint8_t lto, ecc, inter_table, utc_flag;
  uint32_t mjd;
  uint8_t lsi, hours, minutes, seconds;
  uint16_t milliseconds;
  uint8_t pad[6];
  int64_t time_frame;               /* frame of the latest 0/10; -1 without */
  int64_t first_frame, last_frame, changes;
} dabhip_dir_ensemble_rec;
typedef struct dabhip_dir_subch {
  uint8_t have;                     /* DABHIP_DIR_SUB_HAVE_* */
  uint8_t id;
  uint8_t form;                     /* 0 short (UEP), 1 long (EEP) */
  uint8_t uep_index;                /* short form */
  uint8_t protlev;                  /* short: 1..5; long: level | option << 2 */
  uint8_t fec_scheme;               /* 0/14 */
  uint16_t start_cu;
  uint16_t size_cu;
  uint16_t bitrate;                 /* kbit/s */
  uint8_t pad[4];
  int64_t first_frame, last_frame, changes;
} dabhip_dir_subch;
typedef struct dabhip_dir_service {
  uint32_t sid;
  uint8_t pd;
  uint8_t have;                     /* DABHIP_DIR_SVC_HAVE_* */
  uint8_t info;                     /* 0/2: local(1) CAId(3) number of components(4) */
  uint8_t ncomp;
  uint8_t comp[30];                 /* two raw bytes per component */
  uint8_t charset;
  uint8_t pad0;
  uint8_t label[16];
  uint16_t char_flags;
  uint8_t pad[6];
  int64_t first_frame, last_frame, changes;
} dabhip_dir_service;
typedef struct dabhip_dir_pktcomp {
  uint16_t scid;
  uint16_t address;
  uint16_t scca;
  uint8_t subch;
  uint8_t dscty;
  uint8_t dg;
  uint8_t scca_flag;
  uint8_t pad[6];
  int64_t first_frame, last_frame, changes;
} dabhip_dir_pktcomp;
typedef struct dabhip_dir_target {
  int32_t kind;                     /* DABHIP_DIR_MP2 ... */
  int32_t subch;                    /* -1: none */
  int32_t address, dg, dscty, fec;  /* PACKET only, else 0 */
  int32_t scid;                     /* PACKET only, else -1 */
  int32_t primary;                  /* the component's P/S bit */
} dabhip_dir_target;
/* NULL when there is no GPU (dabhip_last_error). */
dabhip_dir *dabhip_dir_create(int device, int nstreams);
void dabhip_dir_destroy(dabhip_dir *d);
/* counts[s] ETI frames of stream s, stream after stream in `frames`, in DEVICE memory when on_device != 0 (no alignment needed), else in host
 * memory.  A push of no frames is legal; one push takes at most 65536 frames in all (3840 bytes of fact slots per frame).  Returns the FIBs
 * with a valid CRC in this call, <0 on error. */
int64_t dabhip_dir_push(dabhip_dir *d, const uint8_t *frames, const int64_t *counts, int on_device);
/* The tables of one stream.  _ensemble returns 0; the others copy min(n, cap) entries (out may be null) and return n: sub-channels with any
 * part, in SubChId order; services and packet components in order of first appearance.  <0 on error. */
int dabhip_dir_ensemble(const dabhip_dir *d, int stream, dabhip_dir_ensemble_rec *out);
int dabhip_dir_subchannels(const dabhip_dir *d, int stream, dabhip_dir_subch *out, int cap);
int dabhip_dir_services(const dabhip_dir *d, int stream, dabhip_dir_service *out, int cap);
int dabhip_dir_packet_components(const dabhip_dir *d, int stream, dabhip_dir_pktcomp *out, int cap);
/* 1 complete, 0 not, <0 on error. */
int dabhip_dir_complete(const dabhip_dir *d, int stream);
/* 0 and *out, or DABHIP_DIR_NO_* (a missing link), or -1 (bad arguments, HIP error). */
int dabhip_dir_resolve(const dabhip_dir *d, int stream, int pd, uint32_t sid, int component, dabhip_dir_target *out);
/* Empties the tables of one stream; its counters and frame numbers go on. */
int dabhip_dir_reset(dabhip_dir *d, int stream);
/* Counters since creation: frames, frames_without_fic, frames_skipped, fibs, fibs_crc_failed, figs, figs_truncated, figs_ignored, facts,
 * facts_changed, overflow_dropped.  Returns 0, <0 on error. */
int dabhip_dir_stats(const dabhip_dir *d, int stream, int64_t *counters11);
/* GPU time of the last push in ms, stage by stage (names: "fibs", "merge"); returns the count. */
int dabhip_dir_stage_ms(const dabhip_dir *d, const char **names, float *ms, int cap);

/* ---- EDI out of ETI (ETSI TS 102 693, the DAB layer, over ETSI TS 102 821: AF packets, PFT) ---------- */
/* A stateful consumer of ETI frames that repackages every frame as an EDI packet on the GPU: the TAG items of the frame in an AF packet with
 * its CRC, and, when asked for, PFT fragments with or without RS(255,207) protection.  Off unless asked for and handled like dabhip_ts: frames
 * are pushed stream by stream, the state of every stream (FCTH, SEQ) carries from push to push, and any cutting of a stream into pushes gives
 * the same bytes.  These rules were written from the standards as remembered, not from a copy of them nor from a second EDI implementation
 * (which marks the points least sure of); what this text, tests/edi_model.py and the kernels agree on is what counts.
 *
 * Multi-byte fields are big-endian.  CRC-16 everywhere is the ETI one: x^16 + x^12 + x^5 + 1, start 0xFFFF, MSB first, result complemented;
 * the nine ASCII bytes "123456789" give 0xD64E.
 *
 * Frames.  ETI(NI), 6144 bytes, numbered per stream from 0 since creation, skipped ones included.  ERR = byte 0, FCT = byte 4, FICF = byte 5
 * >> 7, NST = byte 5 & 0x7F, FP = byte 6 >> 5, MID = (byte 6 >> 3) & 3.  STC entry i is the 4 bytes at 8 + 4 i: SCID 6 bits, SAD 10, TPL 6,
 * STL 10.  MNSC is the 2 bytes at 8 + 4 NST.  The main stream starts at 12 + 4 NST: the FIC (96 bytes) if FICF, then 8 STL bytes per entry in
 * STC order.  A frame is skipped when NST > 64, when FICF = 1 and MID != 1, or when its main stream would run past byte 6140.  A skipped frame
 * gives no packet, counts in `frames_skipped`, consumes no sequence number and is invisible to the FCTH rule.  FSYNC and the frame's own CRCs
 * are not checked.  Every other frame is accepted.
 *
 * TAG items: a name of 4 bytes, a length in BITS as u32, then the value.  In order:
 *   *ptr   64 bits: "DETI", major 0x0000, minor 0x0000.
 *   deti   16 bits ATSTF (= 0) << 15 | FICF << 14 | RFUDF (= 0) << 13 | FCTH << 8 | FCT; 32 bits STAT (= ERR) << 24 | MID << 22 | FP << 19 |
 *          RFA (= 0) << 17 | RFU (= 0) << 16 | MNSC; the 96 FIC bytes when FICF.  48 or 816 bits.
 *   est n  for entry n = 1..NST, named 'e', 's', 't', byte n: 24 bits SCID << 18 | SAD << 8 | TPL << 2 | 0, then the entry's 8 STL bytes (STL 0
 *          gives a 3-byte value).
 * The TAG packet is then padded with zero bytes to a multiple of 8 bytes.
 *
 * FCTH, per stream: the first accepted frame has FCTH 0; an accepted frame whose FCT is below the previous accepted frame's takes
 * (FCTH + 1) mod 20, any other keeps it.
 *
 * AF packet: "AF", LEN u32 = the TAG packet's bytes, padding included, SEQ u16, 0x90 (CRC present, major 1, minor 0), 'T', the TAG packet, the
 * CRC-16 over everything before it; l = LEN + 12 bytes.  SEQ is seq0 for a stream's first accepted frame and grows by 1 mod 65536 per accepted
 * frame.
 *
 * Modes.  0: the AF packet as it is.  1: PFT without FEC: with F = max_frag the packet is cut into f = ceil(l / F) consecutive slices of F
 * bytes, the last one shorter.  2: PFT with RS.
 *
 * PF header: "PF", PSEQ u16 = the AF packet's SEQ, FINDEX u24 from 0, FCOUNT u24, u16 FEC << 15 | ADDR (= 0) << 14 | PLEN, with FEC RSk u8
 * and RSz u8: 12 bytes, 14 with FEC; then HCRC, the CRC-16 over them.  A fragment is its header, the HCRC and PLEN bytes.
 *
 * Mode 2.  c = ceil(l / 207), k = ceil(l / c), z = c k - l.  The packet is padded with z zero bytes and cut into c chunks of k bytes.  The
 * code word of a chunk has 255 bytes, byte j the coefficient of x^(254 - j): the k chunk bytes, then 207 - k zero bytes, then 48 parity bytes,
 * the remainder of (the first 207 bytes) x^48 by g(x) = prod (x + alpha^i), i = 0..47; GF(256) by 0x11D, alpha = 2.  RS block: chunk 0's k
 * bytes, its 48 parity bytes, chunk 1's k bytes, its 48 parity bytes, and so on: B = c (k + 48) bytes.  With m = recover (0..5) and F =
 * max_frag (64..1472): s_max = min(floor(48 c / (m + 1)), F), f = ceil(B / s_max), s = ceil(B / f); byte j of fragment i is block byte
 * j f + i, and 0 where that is >= B; every fragment has PLEN = s, RSk = k, RSz = z.  So any m fragments carry at most 48 bytes of any one code
 * word, and a receiver finds c = floor(f s / (k + 48)).
 *
 * Output, per stream: the packets of the last push in frame order, then fragment order, and one record per packet.  Not done (DESIGN.md
 * section 6): ATST time stamps, RFUD, ADDR, transmission modes other than I, a UDP sender, ETI(NA).  The reverse direction is dabhip_edirx, below. */
typedef struct dabhip_edi dabhip_edi;
typedef struct dabhip_edi_rec {     /* one packet of the last push */
  int64_t offset;                   /* of its first byte among the stream's bytes of the last push */
  int64_t frame;                    /* the frame's number */
  int32_t length;                   /* bytes */
  int32_t findex;                   /* 0 in mode 0 */
  int32_t fcount;                   /* 1 in mode 0 */
  uint16_t seq;
  uint16_t pad;
} dabhip_edi_rec;
typedef struct dabhip_edi_sizes {   /* dabhip_edi_plan */
  int32_t c, k, z;                  /* mode 2, else 0 */
  int32_t B;                        /* bytes cut into fragments: c (k + 48) in mode 2, else l */
  int32_t f;                        /* packets */
  int32_t s;                        /* PLEN of every fragment (mode 1: but the last); l in mode 0 */
} dabhip_edi_sizes;
/* The sizes of one AF packet of l bytes (13 .. 2^20), by the function the kernels use; host only, no GPU needed.  recover counts in mode 2
 * only, max_frag in modes 1 and 2.  Returns 0, <0 when an argument is out of range (dabhip_last_error names it). */
int dabhip_edi_plan(int64_t l, int mode, int recover, int max_frag, dabhip_edi_sizes *out);
/* mode 0..2, recover 0..5 (mode 2), max_frag 64..1472 (modes 1, 2), seq0 0..65535.  NULL when there is no GPU or an argument is out of range
 * (dabhip_last_error). */
dabhip_edi *dabhip_edi_create(int device, int nstreams, int mode, int recover, int max_frag, int seq0);
void dabhip_edi_destroy(dabhip_edi *d);
/* counts[s] ETI frames of stream s, stream after stream in `frames`, in DEVICE memory when on_device != 0 (no alignment needed), else in host
 * memory.  A push of no frames is legal; one push takes at most 131072 frames in all.  Returns the packets of this call, <0 on error. */
int64_t dabhip_edi_push(dabhip_edi *d, const uint8_t *frames, const int64_t *counts, int on_device);
/* The packets of the last push of one stream, in order: copies min(n, cap) records, returns n. */
int64_t dabhip_edi_records(const dabhip_edi *d, int stream, dabhip_edi_rec *out, int64_t cap);
/* Their bytes, packet after packet: copies min(n, cap) bytes, returns n. */
int64_t dabhip_edi_data(const dabhip_edi *d, int stream, uint8_t *dst, int64_t cap);
/* The stream's FCTH and SEQ as after creation; its counters and frame numbers go on. */
int dabhip_edi_reset(dabhip_edi *d, int stream);
/* Counters since creation: frames, frames_skipped, frames_without_fic (accepted frames with FICF = 0), packets, bytes out, chunks encoded.
 * Returns 0, <0 on error. */
int dabhip_edi_stats(const dabhip_edi *d, int stream, int64_t *counters6);
/* GPU time of the last push in ms, stage by stage (names: "plan", "scan", "assemble", "rs", "fragment"); returns the count. */
int dabhip_edi_stage_ms(const dabhip_edi *d, const char **names, float *ms, int cap);

/* ---- EDI in: PFT reassembly, RS(255,207) erasure recovery, ETI frames back ---------------------------- */
/* The receiving half of dabhip_edi: a stateful consumer of EDI packets (datagrams) that gives ETI(NI) frames back, on the GPU, for nstreams
 * streams.  It inverts dabhip_edi: for every frame the engine writes, the frames of edirx(edi(F)) are F byte for byte.  Field layouts, the
 * CRC-16 and the code are those stated above; like them these rules were written without a copy of the standards or a second implementation
 * (DESIGN.md section 6 marks the points least sure of).  tests/edirx_model.py restates them; csrc/edirx_plan.hpp is their text as functions.
 *
 * A packet, given its length n (n < 12: bad).
 *   AF: "AF", LEN u32 with LEN + 12 = n, SEQ u16, byte 8 with (byte & 0xF0) = 0x90 (CRC flag set, major version 1, any minor), then 'T'.  It
 *       is a group of its own: f = 1, FINDEX 0, numbered by SEQ, its payload the whole packet.  Its CRC is judged later, with every AF packet.
 *   PF: "PF", PSEQ u16, FINDEX u24, FCOUNT u24, u16 FEC << 15 | ADDR << 14 | PLEN, with FEC RSk u8 and RSz u8, then HCRC over all bytes in
 *       front of it.  n >= 14, n = 14 + PLEN or 16 + PLEN with FEC; the HCRC right; ADDR = 0; FINDEX < FCOUNT; 1 <= FCOUNT <= 256;
 *       1 <= PLEN <= 1472; with FEC 1 <= RSk <= 207 and c = floor(FCOUNT PLEN / (RSk + 48)) in 1..32 with RSz < c.
 * Anything else is dropped and counted in bad_packets; nothing is read past n.
 *
 * The window, per stream, over its packets in arrival order (every one counts in `packets`), q the packet's SEQ / PSEQ.  The first good packet
 * since creation or reset sets next = q.  d = (q - next) mod 65536.
 *   1. d >= 32768: dropped, `late`.
 *   2. d >= depth: the d - depth + 1 numbers from next on leave the window in order: one with an open group is finalised, one without counts
 *      in `missing`; next = q - depth + 1.  (Work bounded by the open groups.)
 *   3. The packet joins the group of q, which it opens if there is none.  The first packet fixes the kind (AF, PF, PF with FEC), FCOUNT, RSk,
 *      RSz and, with FEC, PLEN; a packet that disagrees is dropped, `mismatched`; one whose FINDEX is held is dropped, `duplicates`.  A group
 *      has at most 8416 payload bytes (32 code words and their padding): a packet whose bytes would lie past that -- FCOUNT PLEN with FEC,
 *      (FINDEX + 1) PLEN without (the last fragment of several excepted, see below), n for AF -- is dropped, `mismatched`, and opens no group.
 *   4. While the group of next is open and complete (all f = FCOUNT fragments held; an AF packet at once): it is finalised, next + 1.  (Also
 *      after a dropped packet.)
 * Ready: complete, or, with FEC, at least f - m_max fragments held, m_max = floor(48 / ceil((RSk + 48) / f)): any m_max fragments hold at most
 * 48 bytes of any code word, and the sender's `recover` is never above m_max.  A group that is ready but not complete waits for its missing
 * fragments until it leaves the window (step 2) or is flushed: a stream without loss is never decoded and none of its fragments is `late`.
 * Finalised while not ready: lost, `groups_incomplete`.  flush finalises the open groups in order and sets next behind the last of them.  reset: as after creation; the
 * counters and the frame numbers go on.  State carries, the held fragments' bytes included: any cutting of a stream's packets into pushes,
 * followed by a flush, gives the same frames, records and counters.
 *
 * A ready group becomes an AF packet.
 *   Without FEC: the fragments in FINDEX order.  The fragments but the last must agree on PLEN, the last have no more, and the whole no more
 *   than 8416 bytes, else `groups_refused` (counted when the group is finalised).
 *   With FEC: block byte j f + i is byte j of fragment i.  Code word w is the block bytes from w (RSk + 48) on: RSk data bytes, then (known)
 *   207 - RSk zero bytes, then 48 parity bytes; byte j of the 255 is the coefficient of x^(254 - j).  Its bytes in missing fragments are its
 *   erasures, at most 48.  A word without erasures is taken as it is.  A word with erasures is filled in by erasure decoding (locator from the
 *   places, Forney, first root alpha^0) and must then have 48 zero syndromes, else the group is lost, `groups_rs_failed`: that is an error
 *   beside the erasures, and no error correction is tried.  The AF packet is the c RSk data bytes without the last RSz.  words_filled and
 *   erasures_filled count over the groups that pass here.
 *   Then: at least 12 bytes, "AF", LEN + 12 = its length, byte 8 and 'T' as above, the CRC-16 right, else `groups_crc_failed`.
 *
 * An AF packet becomes an ETI(NI) frame.  From byte 10 to the CRC, while 8 bytes or more remain: a TAG item: name, length in bits (a multiple
 * of 8, the value inside what remains), value.  At most 7 bytes may remain, all zero.
 *   *ptr   must be 8 bytes beginning "DETI".
 *   deti   once, required: the 2 + 4 bytes as dabhip_edi writes them (ATSTF, FICF, RFUDF, FCTH, FCT; STAT, MID, FP, RFA, RFU, MNSC), then 8
 *          bytes of time stamp when ATSTF (skipped; the frame counts in `with_atst`), 96 FIC bytes when FICF, 3 bytes when RFUDF (skipped);
 *          exactly that long.
 *   est n  n = 1, 2, .. in that order, at most 64: 3 bytes SCID << 18 | SAD << 8 | TPL << 2, then 8 STL bytes: length 3 + 8 STL, STL <= 1023.
 *   Any other item is skipped and, for a frame that comes out, counted in `items_ignored`.
 * Refused (`groups_refused`): a broken walk, no deti, FICF with MID != 1, or 12 + 4 NST + 96 FICF + 8 sum(STL) > 6140.
 * The frame: byte 0 STAT; FSYNC 07 3A B6 for even FCT, F8 C5 49 for odd; FCT; FICF << 7 | NST; FP << 5 | MID << 3 | FL >> 8; FL & 255 with
 * FL = NST + 1 + 24 FICF + 2 sum(STL); the STC entries SCID << 26 | SAD << 16 | TPL << 10 | STL; MNSC; the CRC-16 over bytes 4 .. 9 + 4 NST;
 * the FIC and the sub-channels' bytes; the CRC-16 over them; FF FF; FF FF FF FF; then 0x55 up to byte 6143 (a main stream that ends past
 * byte 6136 cuts the FF bytes short at the frame's end).
 *
 * Not done: correction of errors beside erasures, any use of the time stamps, ADDR, ETI(NA), a UDP socket reader, transmission modes other
 * than I. */
#define DABHIP_EDIRX_COUNTERS 15
typedef struct dabhip_edirx dabhip_edirx;
typedef struct dabhip_edirx_rec {   /* one frame of the last push or flush */
  int64_t frame;                    /* its number among the stream's frames since creation */
  int32_t received;                 /* fragments held when its group was finalised */
  int32_t expected;                 /* FCOUNT; 1 for an AF packet */
  int32_t words_filled;             /* code words that had erasures */
  int32_t erasures_filled;          /* bytes filled in */
  uint16_t seq;
  uint8_t fcth;
  uint8_t fct;
  uint32_t pad;
} dabhip_edirx_rec;
/* depth 1..16: the sequence numbers (groups) kept open per stream.  NULL when there is no GPU or an argument is out of range. */
dabhip_edirx *dabhip_edirx_create(int device, int nstreams, int depth);
void dabhip_edirx_destroy(dabhip_edirx *d);
/* counts[s] packets of stream s, stream after stream; lengths[p] (host memory) the bytes of packet p, a datagram boundary; the packets' bytes
 * concatenated in `data`, in DEVICE memory when on_device != 0 (no alignment needed).  A push of no packets is legal; one push takes at most
 * 2^21 packets and 2^31 - 1 bytes.  Returns the ETI frames this call produced, <0 on error. */
int64_t dabhip_edirx_push(dabhip_edirx *d, const uint8_t *data, const int32_t *lengths, const int64_t *counts, int on_device);
/* Finalises the open groups of one stream (-1: of every stream).  Returns the frames this produced, <0 on error. */
int64_t dabhip_edirx_flush(dabhip_edirx *d, int stream);
/* The frames of the last push or flush of one stream, in the order their groups were finalised: copies min(n, cap) records, returns n. */
int64_t dabhip_edirx_records(const dabhip_edirx *d, int stream, dabhip_edirx_rec *out, int64_t cap);
/* Their bytes, 6144 per record: copies the whole frames that fit in cap bytes, returns n (frames). */
int64_t dabhip_edirx_frames(const dabhip_edirx *d, int stream, uint8_t *dst, int64_t cap);
int dabhip_edirx_reset(dabhip_edirx *d, int stream);
/* Counters since creation, min(cap, 15) of: packets, bad_packets, late, duplicates, mismatched, missing, groups_incomplete, groups_rs_failed,
 * groups_crc_failed, groups_refused, words_filled, erasures_filled, items_ignored, with_atst, frames.  Returns how many, <0 on error. */
int dabhip_edirx_stats(const dabhip_edirx *d, int stream, int64_t *counters, int cap);
/* GPU time of the last push or flush in ms, stage by stage (names: "parse", "window", "gather", "rs", "frame", "emit", "carry"). */
int dabhip_edirx_stage_ms(const dabhip_edirx *d, const char **names, float *ms, int cap);

/* ---- ingest stage: other sample formats and rates -> the canonical cu8 at 2.048 Msps ------------------------------
 * Off unless asked for: a stateful object in front of the decoder that turns nstreams streams of cu8 / cs8 / cs16 / cf32 IQ (I first, little-endian)
 * at an integer sample rate Fin into cu8 at 2,048,000 samples/s in device memory, ready for dabhip_engine_decode(..., on_device = 1) and
 * dabhip_stream_feed(..., on_device = 1).  The arithmetic is integer and stated here in full, so the bytes are those of a plain model
 * (tests/ingest_model.py) and do not depend on how the input is cut into pushes:
 *  1. To the 16-bit domain (int32 x, I and Q alike): cu8 (b - 127) 256 (127: the reference's DC offset, input_sdr.c:61-62); cs8 s 256; cs16 the
 *     value; cf32 rint(clamp(f 32768, -32768, 32767)) in fp32, ties to even, NaN -> 0.
 *  2. Rational resampling: L/M = 2048000/Fin reduced.  Output sample m (64-bit): n0 = floor(m M / L), p = m M mod L,
 *     acc = sum over k < T of taps[p][k] x[n0 + T/2 - k] with x[n] = 0 for n < 0, taps int16 in Q14, T even; v = (acc + 8192) >> 14 (arithmetic
 *     shift).  Output m exists once input sample n0 + T/2 has been pushed.  L/M = 1/1 has no filter (T = 0): v = x.
 *  3. Gain and requantisation: o = clamp(127 + ((v g + 32768) >> 16), 0, 255) in 64-bit, 1 <= g < 2^24.  g = 256 maps 16-bit full scale to 8-bit
 *     full scale: cu8 at 2,048,000 with g = 256 is the identity.
 *  4. Automatic gain (gain = 0 at creation; per stream, fixed for its life): E = sum(I^2 + Q^2) over the stream's first W = 65536 input samples in
 *     the 16-bit domain (an exact uint64), g = clamp(floor(32 65536 / sqrt(E / 2W) + 0.5), 1, 2^24 - 1) in IEEE double on the host, 256 when E = 0:
 *     32 LSB rms per rail, the level the modulator's captures decode at.  A stream's input is held back until W samples are there (32 ms of signal,
 *     at most 512 KB per stream), so the bytes do not depend on the pushes with automatic gain either.
 * The tap table (dabhip_ingest_taps: taps[p][k], L rows of T): a Kaiser (beta 7) windowed sinc, cut-off 1.024 MHz, T = 4 ceil(8 M / L), every phase
 * scaled to sum 16384 with the rounding remainder on its largest tap.  Held to: every phase sums to 16384; sum |taps[p][k]| <= 65535 per phase (then
 * |acc| < 2^31: int32 accumulators); the interleaved prototype (rate L Fin) within +-0.05 dB of DC up to 768 kHz and at or below -60 dB from 1.28 MHz.
 * Rates: 2,048,000 <= Fin <= 10,240,000 whose reduced L is at most 1024 and whose table fits the kernel (65536 bytes as it holds it). */
#define DABHIP_INGEST_CU8 0
#define DABHIP_INGEST_CS8 1
#define DABHIP_INGEST_CS16 2
#define DABHIP_INGEST_CF32 3
typedef struct dabhip_ingest dabhip_ingest;
/* gain: g of step 3, or 0 for the automatic gain.  NULL on a refusal (dabhip_last_error says which) or when there is no GPU. */
dabhip_ingest *dabhip_ingest_create(int device, int nstreams, int format, int64_t rate_hz, uint32_t gain);
void dabhip_ingest_destroy(dabhip_ingest *d);
/* Append nbytes[b] bytes (whole samples: refused otherwise) to stream b: host pointers, or device pointers aligned to a sample when on_device != 0.
 * Synchronous.  Returns the output bytes of all streams, <0 on error; the outputs stay where they are until the next push. */
int64_t dabhip_ingest_push(dabhip_ingest *d, const void *const *src, const size_t *nbytes, int on_device);
/* This push's cu8 of one stream: one contiguous device buffer. */
int dabhip_ingest_output(const dabhip_ingest *d, int stream, const uint8_t **dev, size_t *nbytes);
/* The same bytes copied to the host (cap bytes at most: refused when too small); returns the byte count. */
int64_t dabhip_ingest_read(const dabhip_ingest *d, int stream, uint8_t *dst, size_t cap);
/* g of a stream; 0 while its gain window is open. */
uint32_t dabhip_ingest_gain(const dabhip_ingest *d, int stream);
/* GPU time of the last push in ms (names: "upload", "energy", "resample", "keep"; as dabhip_engine_stage_ms); returns the count. */
int dabhip_ingest_stage_ms(const dabhip_ingest *d, const char **names, float *ms, int cap);
/* Test knob, explicit gain only: exactly as if n samples of value 0 in the 16-bit domain (cu8: bytes of 127) had been pushed to every stream and
 * their outputs discarded -- positions beyond 2^32 within reach of small inputs.  The last push's outputs are gone afterwards. */
int dabhip_ingest_skip(dabhip_ingest *d, int64_t n);
/* Without a GPU: the table of a rate (taps may be NULL: only L, M, T; cap in taps) -- returns L T, <0 on a refusal -- */
int dabhip_ingest_taps(int format, int64_t rate_hz, int16_t *taps, int cap, int *L, int *M, int *T);
/* -- the bookkeeping of one stream over a sequence of npush pushes of push_samples[i] samples: nout[i] = output samples push i completes,
 * carried[i] = input samples kept behind it (T - 1, or all of them while the gain window is open) -- and the gain rule of step 4. */
int dabhip_ingest_plan(int64_t rate_hz, int auto_gain, const int64_t *push_samples, int npush, int64_t *nout, int64_t *carried);
uint32_t dabhip_ingest_auto_gain(uint64_t energy);

/* ---- ingest stage, tuned mode: several DAB blocks out of one wideband capture -------------------------------------
 * dabhip_ingest_create_tuned makes an ingest object with a mixer in front of the resampler: each of nstreams input streams gives nchannels output
 * streams, channel c being the block whose centre lies offsets_hz[c] Hz from the capture's centre (signed; Band III blocks are 1,712,000 Hz apart),
 * brought to 0 Hz and resampled to the canonical cu8.  Objects of dabhip_ingest_create are not touched by any of this.  The arithmetic is integer,
 * stated here in full (the plain model of it: tests/tune_model.py), and its bytes do not depend on how the input is cut into pushes:
 *  1. To the 16-bit domain: step 1 above, for all four formats (cu8's 255 gives 32768: x is an int32).
 *  2. Mixer.  For the channel's offset f and the input rate Fin, step = floor((2 f 2^32 + Fin) / (2 Fin)) mod 2^32 in exact integers, floor towards
 *     minus infinity (f / Fin of a turn in units of 2^-32 turn, rounded to nearest; dabhip_ingest_tune_step).  For the input sample at absolute 64-bit
 *     position n of its stream (the first sample ever pushed is n = 0; dabhip_ingest_skip advances n): theta = (n step) mod 2^32,
 *     i = ((theta + 2^19) mod 2^32) >> 20, a 12-bit index (a theta within 2^19 of a full turn gives i = 0).  The table (dabhip_ingest_tune_nco) has
 *     4096 pairs of int16: c[i] = rint(16384 cos(2 pi i / 4096)), s[i] = rint(16384 sin(2 pi i / 4096)), the quarter points exact (+-16384 and 0).
 *       yI = clamp((xI c[i] + xQ s[i] + 8192) >> 14, -32768, 32767),  yQ = clamp((xQ c[i] - xI s[i] + 8192) >> 14, -32768, 32767)
 *     with arithmetic shifts: y = x e^(-j theta), so a block centred at +f lands at 0.  The phase is a function of n alone, nothing accumulates.  The
 *     clamp is real: a full-scale sample at 45 degrees reaches 46341.
 *  3. Resampling: step 2 above on y (y[n] = 0 for n < 0), with the TUNED table (dabhip_ingest_tune_taps): the same construction with
 *     T = 8 ceil(8 M / L) taps per phase (twice the plain table's), the -6 dB point at 856 kHz, Kaiser beta 7, every phase scaled to sum 16384 with
 *     the rounding remainder on its largest tap.  Held to: every phase sums to 16384; sum |taps[p][k]| <= 65535 per phase; the interleaved
 *     prototype within +-0.05 dB of DC up to 768 kHz and at or below -60 dB from 944 kHz (1,712,000 - 768,000: where the neighbouring block begins).
 *     Fin = 2,048,000 has no filter (T = 0): v = y.
 *  4. Gain and requantisation: step 3 above.
 *  5. Automatic gain (gain = 0 at creation), per OUTPUT stream and fixed for its life: E = sum(vI^2 + vQ^2) over the channel's first W = 65536
 *     outputs v of step 3 (an exact uint64), g = dabhip_ingest_auto_gain(E).  All channels of an input stream are held back, and all of its input is
 *     carried, until its pushed input completes output 65535 (input sample floor(65535 M / L) + T/2); that push delivers outputs from 0 on.  The
 *     energy of the wideband input would be the wrong measure: a weak block beside a strong one must still fill its 8 bits.
 * Refused: fewer than 1 or more than 16 channels; an offset with |f| + 768,000 > Fin / 2 (the block does not lie within the capture);
 * nstreams nchannels > 65535; a rate dabhip_ingest_create refuses; a rate whose tuned table, input tile and NCO table (16 KiB) do not fit the 160 KiB
 * of LDS one workgroup has on gfx950 (10,000,000 Hz: 82,432 + 21,288 + 16,384 bytes, taken; 10,229,760 Hz is the kind that is not).
 * Output stream `stream nchannels + channel` is what dabhip_ingest_output, _read and _gain call `stream`; dabhip_ingest_push still takes one input
 * per INPUT stream and returns the output bytes of all output streams; _skip and _stage_ms are as above. */
dabhip_ingest *dabhip_ingest_create_tuned(int device, int nstreams, int format, int64_t rate_hz, uint32_t gain, const int64_t *offsets_hz, int nchannels);
/* Without a GPU: the tuned table of a rate (as dabhip_ingest_taps) -- */
int dabhip_ingest_tune_taps(int format, int64_t rate_hz, int16_t *taps, int cap, int *L, int *M, int *T);
/* -- the mixer's table, cs[2 i] = c[i], cs[2 i + 1] = s[i] (cap in pairs, 4096 at least); returns 4096 -- */
int dabhip_ingest_tune_nco(int16_t *cs, int cap);
/* -- the step of an offset at a rate; returns 0, <0 when the rate or the offset is refused -- */
int dabhip_ingest_tune_step(int64_t rate_hz, int64_t offset_hz, uint32_t *step);
/* -- and the bookkeeping of one input stream as dabhip_ingest_plan gives it: nout[i] = output samples push i completes in EVERY channel,
 * carried[i] = input samples kept behind it (T - 1 or all there are; everything while the gain window is open, which closes on outputs). */
int dabhip_ingest_tune_plan(int64_t rate_hz, int auto_gain, const int64_t *push_samples, int npush, int64_t *nout, int64_t *carried);

/* ---- block scan: which DAB blocks lie in a wideband capture ------------------------------------------------------
 * Off unless asked for: a stateful object that measures the power spectrum of the beginning of nstreams streams of cu8 / cs8 / cs16 / cf32 IQ at an
 * integer sample rate Fin, and a host rule that turns such a spectrum into the list of Mode-I blocks (1.536 MHz wide) in it, as offsets from the
 * capture's centre that dabhip_ingest_create_tuned takes.  Nothing of the decoder or of the ingest objects is touched.  The arithmetic is integer and
 * stated here in full, so the spectrum is that of a plain model (tests/scan_model.py), bit for bit, however the input is cut into pushes:
 *  0. Window.  S = 4096 samples are a segment; the scan window of a stream is its first nsegments complete segments, counted from the first sample
 *     ever pushed.  Samples past the window are ignored; a stream with fewer than S samples has 0 segments and an all-zero spectrum.
 *  1. Samples: step 1 of the ingest stage, all four formats (cu8's 255 gives 32768: x is an int32).
 *  2. Transform, per segment: radix-2 decimation in time on the bit-reversed segment (v[i] = x[bit-reverse12(i)]) with the tuned mode's NCO table
 *     c[i], s[i] (dabhip_ingest_tune_nco: 4096 entries in Q14).  Stages of half size h = 1, 2, 4, ..., 2048; the butterfly of a stage takes a at index
 *     i and b at index i + h (i mod 2h < h), with q = i mod h and table index t = q (2048 / h):
 *       tI = (bI c[t] + bQ s[t] + 8192) >> 14,   tQ = (bQ c[t] - bI s[t] + 8192) >> 14      (the mixer's product b e^(-j theta): arithmetic shifts, no clamp)
 *       a' = (a + t + 1) >> 1,   b' = (a - t + 1) >> 1                                      (per rail)
 *     Every stage halves, so X[k] is about (1/4096) sum x[n] e^(-2 pi j k n / 4096), in transform order (bin k: frequency k Fin / 4096, k >= 2048
 *     negative).  These two roundings per butterfly are the only ones; everything else is exact, so the order of work cannot matter.
 *  3. Power: P[k] = sum over the window's segments of XI[k]^2 + XQ[k]^2, an exact uint64 (at most about 2^32 per segment and bin).
 *  4. Range.  Every intermediate value stays within +-46,400 per rail: the magnitude of a sample is at most 32768 sqrt 2 = 46,341 (full scale on both
 *     rails); a butterfly gives |a'|, |b'| <= (|a| + |t|) / 2 + 1 with |t| <= |b| |w| / 16384 + 1, where |w| <= 16384 (1 + 2^-14) for every entry of
 *     the rounded table (c^2 + s^2 <= 16384^2 + 16384 sqrt 2 + 1/2): a stage takes the largest magnitude M to at most M (1 + 2^-15) + 3/2, which adds
 *     less than 3, 12 stages less than 36.  A rail is no larger than the magnitude.  Both products of tI or tQ together are at most |b| |w| < 46,400 16,385 < 2^30, plus 8192 still below 2^31: int32 arithmetic
 *     suffices, and both factors of every product fit 24 bits.
 * From spectrum to blocks (dabhip_scan_detect; integers, 128-bit products).  Shifted index b = (k + 2048) mod 4096 has frequency
 * (b - 2048) Fin / 4096; sums below are over P in shifted order.  ni = floor(700000 4096 / Fin), a0 = ceil(800000 4096 / Fin),
 * a1 = floor(900000 4096 / Fin), w = max(1, floor(16000 4096 / Fin)), nin = 2 ni + 1, ng = a1 - a0 + 1.
 *  - Candidates: for every centre bin c in [a1, 4096 - a1): in(c) = sum over [c - ni, c + ni], lo(c) = sum over [c - a1, c - a0], hi(c) = sum over
 *    [c + a0, c + a1] (the middle of the 176 kHz guard either side of a block).  c is a candidate when in ng > 4 lo nin and in ng > 4 hi nin: the
 *    in-band mean more than 6 dB above both guards' (strict: an all-zero spectrum has no candidate).
 *  - Runs: each maximal run [a, b] of consecutive candidates is one detection; raw_center_hz = floor(((a + b - 4096) Fin + 4096) / 8192).
 *  - Edges: c = (a + b) div 2, in = in(c).  Towards each side d = -1, +1, j walks from c + d ni in steps of d; the box of j is
 *    [max(0, j - w), min(4096, j + w + 1)), s its sum and n its bin count.  The walk stops at the first j with 4 s nin < in n (the box mean below a
 *    quarter of the in-band mean), or at j = 0 or j = 4095: that j is the edge e_d.  offset_hz = floor(((e- + e+ - 4096) Fin + 4096) / 8192),
 *    width_hz = floor((e+ - e-) Fin / 4096).  (The run centre alone is pulled several kHz by a strong neighbour; the edges are not.)
 *  - Width gate: kept only when 1,436,000 <= width_hz <= 1,636,000.
 *  - Raster, when center_hz > 0 (the capture's centre frequency; 0 = not known): if the nearest of the 38 Band III block centres (5A 174,928 kHz, B, C,
 *    D each + 1712; the same from 6A 181,936, 7A 188,928, 8A 195,936, 9A 202,928, 10A 209,936, 11A 216,928, 12A 223,936; 13A 230,784, 13B 232,496,
 *    13C 234,208, 13D 235,776, 13E 237,488, 13F 239,200) is within 32,000 Hz of center_hz + offset_hz, offset_hz becomes that centre minus center_hz
 *    exactly and the block carries its name; otherwise the measured offset stays and the name is empty.
 *  - The blocks in ascending offset, 16 at most: more is an error that names the count.
 * Reach, as far as a plain model of all this was run on synthetic captures: a block down to 20 dB below its neighbour, about 5 dB of in-band SNR.
 * Levels in dB are for display (10 log10 of in / nin and of the ratio to the guards) and enter no decision. */
typedef struct dabhip_scan dabhip_scan;
typedef struct dabhip_scan_block {
  int64_t offset_hz;       /* the block's centre from the capture's centre: measured from the edges, or exact when snapped to the raster */
  int64_t raw_center_hz;   /* the run's centre */
  int64_t width_hz;
  uint64_t in, lo, hi;     /* the sums of the run's centre bin: in over nin bins, lo and hi over ng bins each (saturating at 2^64 - 1, which no
                              spectrum of a scan object reaches) */
  int32_t nin, ng;
  char name[8];            /* "5A" .. "13F", or "" */
} dabhip_scan_block;
#define DABHIP_SCAN_BINS 4096
#define DABHIP_SCAN_DEFAULT_SEGMENTS 64
/* nsegments: 1 .. 65536.  Rates: any integer from 2,048,000 to 10,240,000 (no table depends on the rate).  NULL on a refusal or without a GPU. */
dabhip_scan *dabhip_scan_create(int device, int nstreams, int format, int64_t rate_hz, int nsegments);
void dabhip_scan_destroy(dabhip_scan *d);
/* Append nbytes[b] bytes (whole samples: refused otherwise) to stream b: host pointers, or device pointers aligned to a sample when on_device != 0.
 * The up to 4095 samples of an unfinished segment are carried.  Synchronous.  Returns the segments accumulated by this push over all streams, <0 on
 * error. */
int64_t dabhip_scan_push(dabhip_scan *d, const void *const *src, const size_t *nbytes, int on_device);
/* P of one stream (4096 bins in transform order) and the segments it holds so far. */
int dabhip_scan_spectrum(const dabhip_scan *d, int stream, uint64_t *P, int *nsegments_done);
/* dabhip_scan_spectrum followed by dabhip_scan_detect: copies min(n, cap) records, returns n, <0 on error. */
int dabhip_scan_blocks(const dabhip_scan *d, int stream, int64_t center_hz, dabhip_scan_block *out, int cap);
/* GPU time of the last push in ms (names: "upload", "transform", "keep"; as dabhip_engine_stage_ms); returns the count. */
int dabhip_scan_stage_ms(const dabhip_scan *d, const char **names, float *ms, int cap);
/* Without a GPU: the rule above on a spectrum of 4096 bins.  Copies min(n, cap) records, returns n, <0 on error (rate outside 2,048,000 ..
 * 10,240,000, center_hz negative or above 10^12, more than 16 blocks). */
int dabhip_scan_detect(const uint64_t *P, int64_t rate_hz, int64_t center_hz, dabhip_scan_block *out, int cap);
/* -- and the bookkeeping of one stream over a sequence of pushes: nseg[i] = segments push i completes, carried[i] = samples kept behind it. */
int dabhip_scan_plan(int nsegments, const int64_t *push_samples, int npush, int64_t *nseg, int64_t *carried);

/* ---- TII: which transmitters a received ensemble comes from ------------------------------------------------------
 * Off unless asked for (dabhip_engine_set_tii / dabhip_stream_set_tii): the decoder otherwise uses the null symbol for coarse timing only.  In a
 * Mode-I single-frequency network every transmitter marks the null symbol of every second transmission frame with its own comb of carriers (ETSI
 * EN 300 401, clause 14.8): a main identifier 0 .. 69 and a sub identifier 0 .. 23.  With TII on, a decode transforms a window of the null symbol of
 * every demodulated frame, folds the power onto 24 x 8 sums per stream, and a host rule reads the identifiers off the sums.  ETI bytes, traces,
 * operator text and stage names are those of a decode without it.  The arithmetic is integer and stated here in full, so the sums are those of a
 * plain model (tests/tii_model.py), bit for bit, whatever the launch shape:
 *  0. Patterns and carriers.  The 70 patterns are the 8-bit words with exactly four ones in ascending numeric order (pattern 0 = 0x0f, pattern 69 =
 *     0xf0); a_b(p) is bit 7 - b of word p, b = 0 .. 7.  Transmitter (p, c) sends, for every b with a_b(p) = 1 and every quarter base in {-768, -384,
 *     1, 385}, the carrier pair k = base + 2 c + 48 b and k + 1: 32 carriers (dabhip_tii_carriers), both of a pair with the phase-reference phase of
 *     the lower one (the standard's A(k) e^(j phi_k) + A(k-1) e^(j phi_(k-1))).  Over c, b, the quarters and the two carriers these tile the 1536
 *     carriers exactly once.
 *  1. Frames counted.  A demodulated call (what dabhip_engine_trace reports as ok) counts when |fine_timeshift| <= 304 and
 *     |fine_freq_shift| < 1,024,000 (a NaN does not count; no estimate of the front end comes near the bound, it only keeps step 3 in range).
 *  2. Window and samples.  2048 samples of the call's frame buffer from sample w0 = 304 + fine_timeshift on (0 <= w0 <= 608: the TII symbol has
 *     period 2048 over the 2656 samples of the null symbol, so every such window holds one period); x = (byte - 127) 128 per rail.
 *  3. De-rotation.  f = 1000 coarse_freq_shift + fine_freq_shift + nco_hz in Hz (doubles, added left to right; nco_hz: dabhip_engine_trace_nco,
 *     0 without the software AFC) -- the capture's carrier offset as the front end measured it, same sign as dabhip_synth_cfg.cfo_hz.
 *     step = nearbyint(f 4294967296.0 / 2048000.0) mod 2^32 (doubles, left to right, ties to even); theta_n = (step n) mod 2^32 with n counted from
 *     the window's first sample; table index i = ((theta_n + 2^19) mod 2^32) >> 20 into dabhip_ingest_tune_nco;
 *       yI = (xI c[i] + xQ s[i] + 8192) >> 14,   yQ = (xQ c[i] - xI s[i] + 8192) >> 14      (the tuned mode's product, arithmetic shifts, no clamp)
 *  4. Transform: the block scan's step 2 with 2048 points -- on the bit-reversed window (v[i] = y[bit-reverse11(i)]), stages of half size h = 1, 2,
 *     ..., 1024, table index t = q (2048 / h) in the same 4096-entry table, the same butterfly with its two roundings.  X[k] is about
 *     (1/2048) sum y[n] e^(-2 pi j k n / 2048).
 *  5. Range: the block scan's step 4 with half the input range.  |x| <= 16384 per rail, a magnitude of at most 16384 sqrt 2 = 23,171; the
 *     de-rotation gives at most 23,171 (1 + 2^-14) + 1 < 23,175, and 11 stages add less than 33: every value stays within +-23,210 per rail, both
 *     products of a sum together below 23,210 x 16,385 < 2^29: int32 arithmetic and 24-bit factors hold a fortiori.
 *  6. Fold.  Carrier k lies in bin k mod 2048.  T[c][b] += XI^2 + XQ^2 over the eight bins of (c, b) -- four quarters times two carriers -- of every
 *     counted frame: exact uint64 sums (at most about 2^32 per frame and sum), so neither launch shape nor order can matter.  T is stored as
 *     T[8 c + b], 192 values.
 * From sums to identifiers (dabhip_tii_detect; integers, 128-bit products).  For each c: order the eight T[c][b] descending, ties to the lower b:
 * v0 .. v7; s = v0 + v1 + v2 + v3, n = v4 + .. + v7.  The comb is present when s > 2 n and v3 > 2 v4 (both strict: an all-zero T yields nothing); its
 * main identifier is the index of the word made of the four strongest b.  DABHIP_TII_SHADOW flags a comb when another present comb has the same main
 * identifier and an s more than 64 times larger: the leakage of a strong comb under a residual frequency error looks like that -- flagged, not
 * dropped, because a real weak transmitter of the same main identifier looks the same.  Records come out in ascending c, 24 at most.  Several
 * transmitters that share one sub identifier are NOT separated: their combs add, and the rule sees the four strongest b of the sum or nothing.
 * Reach, as far as a plain model of all this was run on the modulator's captures (28 LSB rms per rail, TII in every second frame): one transmitter
 * at the level of a data carrier from 8 frames on at 5 dB, transmitters 10 and 20 dB below the strongest in 16 clean frames, nothing in noise alone
 * at 5 dB in 2 and in 8 frames.  The rule compares a comb with the bins around it and does not subtract the noise floor, so noise bounds its reach
 * however many frames are folded: at 9 dB a comb at the level of a data carrier beside one 10 dB stronger is found from 4 frames on and a comb 4 dB
 * below a data carrier from 6 frames on, a comb 7 dB or more below a data carrier never.  Levels in dB are for display and enter no decision. */
#define DABHIP_TII_SUMS 192
#define DABHIP_TII_SHADOW 1u
typedef struct dabhip_tii_id {
  int32_t main_id;         /* 0 .. 69 */
  int32_t sub_id;          /* 0 .. 23 */
  uint32_t flags;          /* DABHIP_TII_SHADOW */
  int32_t pad;
  uint64_t strong, weak;   /* s and n of the rule (saturating at 2^64 - 1, which no sum of a decode reaches) */
} dabhip_tii_id;
/* enable != 0: every later decode also runs the TII stage: one kernel over the decode's calls, on the engine's stream behind the OFDM stage's launches. */
int dabhip_engine_set_tii(dabhip_engine *e, int enable);
/* The sums of one stream of the last decode (zero when it began) and the frames that counted; either pointer may be NULL. */
int dabhip_engine_tii_sums(dabhip_engine *e, int stream, uint64_t *T, int *frames);
/* dabhip_engine_tii_sums followed by dabhip_tii_detect: copies min(n, cap) records, returns n, <0 on error. */
int dabhip_engine_tii(dabhip_engine *e, int stream, dabhip_tii_id *out, int cap);
/* GPU time of the TII kernel in the last decode in ms (HIP events); 0 when it did not run.  Not among dabhip_engine_stage_ms's names. */
int dabhip_engine_tii_ms(const dabhip_engine *e, float *ms);
/* The same for a session: the sums accumulate over the session's segments until dabhip_stream_tii_reset. */
int dabhip_stream_set_tii(dabhip_stream *s, int enable);
int dabhip_stream_tii_sums(dabhip_stream *s, int stream, uint64_t *T, int *frames);
int dabhip_stream_tii(dabhip_stream *s, int stream, dabhip_tii_id *out, int cap);
int dabhip_stream_tii_reset(dabhip_stream *s);
/* Without a GPU: the rule above on 192 sums.  Copies min(n, cap) records, returns n (0 .. 24), <0 on error (T NULL, cap < 0, out NULL with cap > 0). */
int dabhip_tii_detect(const uint64_t *T, dabhip_tii_id *out, int cap);
/* -- and the 32 carriers (-768 .. 768 without 0) of transmitter (main_id, sub_id), quarter after quarter, ascending within each.  Returns 32,
 * <0 on error (no such transmitter, k NULL, cap < 32). */
int dabhip_tii_carriers(int main_id, int sub_id, int16_t *k, int cap);
/* Stage entry (parity tests): steps 2 - 6 on nframes contiguous frames of 393216 bytes (device pointer when on_device) with explicit window starts
 * w0[j] (0 .. 608, refused otherwise) and steps step[j] (host arrays) -> T[nframes][192] (host), one T per frame. */
int dabhip_stage_tii(dabhip_engine *e, const uint8_t *frames, int nframes, const int32_t *w0, const uint32_t *step, int on_device, uint64_t *T);

/* ---- synthetic Mode-I modulator (host only) --------------------------------------------- */
typedef struct dabhip_subch_cfg {
  int32_t id;          /* SubChId 0..63 */
  int32_t start_cu;    /* 0..863 */
  int32_t slform;      /* 0 = UEP (uep_index), 1 = EEP (eep_protlev, size_cu) */
  int32_t uep_index;   /* 0..63, ETSI Table 7 */
  int32_t eep_protlev; /* option<<2 | level: 0..3 = 1-A..4-A, 4..7 = 1-B..4-B */
  int32_t size_cu;     /* EEP only */
} dabhip_subch_cfg;

typedef struct dabhip_reconf_cfg {
  int32_t at_cif;        /* logical CIF index from which the MSC carries this multiplex; 0 = entry unused */
  int32_t fic_lead;      /* the FIC signals it this many CIFs earlier (>= 0) */
  int32_t nsub;
  int32_t pad;
  dabhip_subch_cfg sub[64];
} dabhip_reconf_cfg;

/* Order of application to the modulator's complex samples x[n] (n counts from the capture's first sample, skipped ones included):
 * echoes, fading, carrier offset (cfo_hz above), sample-rate offset, I/Q imbalance; then skip_samples, noise and the cu8 quantisation as before. */
typedef struct dabhip_channel_cfg {
  double sro_ppm;          /* the receiver's sample clock against the transmitter's: output sample m is the signal at input position m (1 + ppm 1e-6)
                              (windowed-sinc interpolation, 16 taps): > 0 = frames arrive SHORTER than 196,608 samples (negative time shifts) */
  int32_t echo_delay[2];   /* two-ray / three-ray multipath: x[n] += gain e^(2 pi i (phase + doppler n / 2.048e6)) x[n - delay]; delay in samples, 0 = no echo, <= 2047 */
  double echo_gain[2];     /* linear, relative to the direct path */
  double echo_phase[2];    /* turns */
  double echo_doppler_hz[2];
  double fade_depth;       /* slow flat fading: amplitude 1 - depth (1 - cos(2 pi fade_hz t)) / 2, 0 <= depth < 1 */
  double fade_hz;
  double iq_gain_db;       /* receiver imbalance: Q rail gain over I rail */
  double iq_phase_deg;     /* quadrature error: Q' = g (Q cos phi + I sin phi) */
} dabhip_channel_cfg;

typedef struct dabhip_tii_cfg {
  int32_t enabled;
  int32_t main_id;         /* 0 .. 69 */
  int32_t sub_id;          /* 0 .. 23 */
  int32_t pad;
  double level_db;
} dabhip_tii_cfg;

typedef struct dabhip_synth_cfg {
  uint32_t eid;
  int32_t nsub;
  dabhip_subch_cfg sub[64];
  uint64_t seed;          /* payload / filler / noise seed */
  int32_t cif_count0;     /* CIF counter of the first CIF, 0..4999 */
  int32_t skip_samples;   /* drop this many samples from the start (0..196607): unaligned capture */
  double amplitude;       /* LSB per unit carrier of the unnormalised IDFT (1.0 -> ~28 LSB rms per rail) */
  double snr_db;          /* signal/noise power over the 2.048 MHz band; >= 100 -> no noise */
  double cfo_hz;          /* carrier frequency offset applied to the whole capture (0 = none) */
  /* Test vectors for FIC content the presets do not produce (non-standard or hostile FIGs): when fib_patch_len > 0, the THIRD FIB of every CIF
   * from fib_patch_from_cif on carries these bytes (FIGs, then end marker / padding) under a VALID CRC -- what a corrupted FIB that passes the
   * 16-bit CRC looks like to fib_parse (fic.c:47-130).  The MSC content is unaffected.  0-initialised = off. */
  int32_t fib_patch_len;  /* 0..30 */
  int32_t fib_patch_from_cif;
  uint8_t fib_patch[32];
  /* Multiplex reconfigurations (round 5): from logical CIF reconf[k].at_cif on (counted from the capture's first CIF; 0 = unused; ascending) the MSC
   * carries the sub-channels reconf[k].sub[0..nsub) instead, and the FIG 0/1 entries of the FIC announce them from CIF at_cif - fic_lead on.  The
   * reference knows nothing of ETSI's reconfiguration signalling: merge_info (misc.c:14-27) overwrites the slots of the SubChIds it hears and never
   * removes one, on every locked TF BEFORE the oldest CIFs of the ring are emitted (dab.c:64-97) -- frames already in the ring are laid out by the new
   * FIG 0/1.  Whatever that yields is the parity target.  dabhip_synth_payload's slot then indexes the multiplex in force at that CIF. */
  dabhip_reconf_cfg reconf[2];
  /* Channel between modulator and receiver (round 5; all zero = the ideal channel of rounds 1-4, byte-identical captures).  Host generator only:
   * dabhip_synth_generate_device refuses a configuration with any of these set. */
  dabhip_channel_cfg channel;
  /* DAB+ content (ETSI TS 102 563; all zero = off, byte-identical captures): bit k set = slot k carries audio superframes instead of keyed
   * random bytes.  Superframe n of a slot spans logical CIFs dabplus_phase + 5 n .. + 4 (n may be negative: every CIF belongs to one).  Each slot
   * draws its audio parameters from its key -- consecutive slots cycle through the four (dac_rate, sbr_flag) pairs, i.e. 2 / 3 / 4 / 6 AUs --
   * and each superframe its AU lengths and content; the synth computes the AU CRCs, the fire code and the RS parity, and interleaves.  The
   * slots' bit rates must be multiples of 8 kbit/s; refused together with reconfigurations. */
  uint64_t dabplus_slots;
  int32_t dabplus_phase;
  /* TII (see "TII" above; all zero = off, byte-identical captures): transmission frames tf (counted from the capture's first) with tf + tii_phase
   * even carry, in the 2656 samples of their null symbol, the sum of the enabled combs: amplitude sum over the comb's carriers k of
   * 10^(level_db / 20) e^(j phi) e^(2 pi j k (n - 608) / 2048), phi the phase-reference phase of the pair's lower carrier.  level_db is relative to a
   * data carrier.  The other frames' null symbols stay silent; the noise draws do not move.  Host generator only: dabhip_synth_generate_device
   * refuses a configuration with TII set. */
  int32_t tii_phase;
  dabhip_tii_cfg tii[4];
  /* Packet-mode content (see "packet-mode data" above; all zero = off, byte-identical captures): bit k of packet_slots set = slot k carries packets
   * instead of keyed random bytes; bit k of packet_fec_slots (a subset) = with the FEC frames of the enhanced packet mode.  With FEC, frame j of a
   * slot starts at cell 103 j + packet_phase, cells counted from logical CIF 0's first (j may be negative: every cell belongs to a frame); without,
   * every logical CIF's cells are a unit.  Each unit is filled from the slot's key: data groups with random lengths and flags, which start and end
   * inside the unit, cut into packets of mixed lengths on two or three addresses, command packets in between, padding packets to fill it exactly;
   * then the parity.  The slots' bit rates must be multiples of 8 kbit/s; refused on a DAB+ slot, on a slot past nsub, and together with
   * reconfigurations. */
  uint64_t packet_slots;
  uint64_t packet_fec_slots;
  int32_t packet_phase;
  int32_t packet_pad;
  /* MPEG-2 TS content (see "MPEG-2 transport stream" above; all zero = off, byte-identical captures): bit k of ts_slots set = slot k carries an
   * interleaved transport stream instead of keyed random bytes.  The slot of code word n starts at byte 204 n + ts_phase, bytes counted from
   * logical CIF 0's first (n may be negative: the interleaver has run forever, so every byte belongs to a word).  Each word is made from the
   * slot's key: 0x47, two or three PIDs and null packets in between, a continuity counter per PID, a keyed payload, the
   * payload_unit_start_indicator now and then; then the parity.  Any bit rate; refused on a DAB+ slot, on a packet-mode slot, on a slot past
   * nsub, and together with reconfigurations.  Host generator only: dabhip_synth_generate_device refuses a configuration with ts_slots set. */
  uint64_t ts_slots;
  int32_t ts_phase;
  int32_t ts_pad;
  /* Service information (see "ensemble directory" above; 0 = off, byte-identical captures and dabhip_synth_fibs).  1: the room that FIG 0/0 and
   * FIG 0/1 leave in the three FIBs of a CIF carries a carousel of whole FIGs, in this order: FIG 1/0 "DABHIP SYNTH"; FIG 0/9 (LTO 0, ECC 0xE1,
   * table 1); FIG 0/10 (long form: MJD 60000 at 00:00:00.000 UTC plus 24 ms x (cif_count0 + CIF index)); then for every slot k a service --
   * SId 0x1000 + k, P/D 0 for a plain (MP2) or DAB+ slot, SId 0xE0001000 + k, P/D 1 for a ts_slots or packet_slots slot -- as a FIG 0/2 entry
   * with one primary component (plain: TMId 0, ASCTy 0; DAB+: TMId 0, ASCTy 63; TS: TMId 1, DSCTy 24; packet: TMId 3, SCId k), its label FIG
   * 1/1 or 1/5 "SLOT kk KIND" (kk in two decimal digits; KIND = MP2, DAB+, TS, PACKET; padded with spaces to 16; charset 0, flag field 0xFF00)
   * and, for a packet slot, a FIG 0/3 entry (SCId k, the slot's SubChId, its first address as dabhip_synth_packet_addresses gives it, DG flag
   * 1, DSCTy 60, no SCCA) and, when packet_fec_slots names it, a FIG 0/14 byte with scheme 1.  The carousel is cut into loads: a load takes FIGs
   * in order, each into the first FIB with room; the first that fits nowhere starts the next load; CIF c carries load c mod the number of loads.
   * A FIG never splits.  Refused together with reconfigurations, with fib_patch_len > 0, and when a FIG fits in no FIB.  Both generators honour
   * it: the device modulator takes its FIBs from the same host function. */
  int32_t si_mode;
  int32_t si_pad;
} dabhip_synth_cfg;

/* preset 0: 12 sub-channels, 1136 kbit/s, 862 CU (the benchmark mix); 1: 4 light sub-channels. */
int dabhip_synth_preset(int preset, dabhip_synth_cfg *cfg);
/* Bytes dabhip_synth_generate writes for ntf transmission frames -- exactly that with channel.sro_ppm == 0; with a sample-rate offset an upper
 * bound (the capacity to pass), the call's return value being the count. */
size_t dabhip_synth_bytes(const dabhip_synth_cfg *cfg, int ntf);
/* Generate ntf transmission frames of cu8 IQ into iq (capacity cap bytes). Returns bytes written or <0. */
int64_t dabhip_synth_generate(const dabhip_synth_cfg *cfg, int ntf, uint8_t *iq, size_t cap);
/* The payload (before energy dispersal) carried by sub-channel slot k in logical CIF n:
 * bitrate*3 bytes.  Returns the byte count, <0 on error. */
int dabhip_synth_payload(const dabhip_synth_cfg *cfg, int cif_index, int slot, uint8_t *out, int cap);
/* The 96 FIB bytes (3 FIBs with CRC) carried by CIF n. */
int dabhip_synth_fibs(const dabhip_synth_cfg *cfg, int cif_index, uint8_t *out96);
/* The unprotected 110 s bytes of DAB+ superframe sf_index of slot (a dabplus_slots slot of 8 s kbit/s): fire code, header, au_start, the AUs
 * with their CRCs -- before the RS parity and the interleaving that dabhip_synth_payload's bytes carry.  Returns 110 s, <0 on error. */
int dabhip_synth_dabplus_superframe(const dabhip_synth_cfg *cfg, int sf_index, int slot, uint8_t *out, int cap);
/* Truth of a packet-mode slot, straight from the generator (not through dabhip_packet): the addresses its groups go out on (2 or 3, returns the
 * count); ncells transmitted cells from cell_index on (cells counted from logical CIF 0's first; returns 24 ncells); the n-th data group of an
 * address, counted from unit 0 on (FEC frame 0, or logical CIF 0 without FEC): min(length, cap) bytes, returns the length.  <0 on error. */
int dabhip_synth_packet_addresses(const dabhip_synth_cfg *cfg, int slot, int32_t *out3);
int dabhip_synth_packet_cells(const dabhip_synth_cfg *cfg, int slot, int64_t cell_index, int ncells, uint8_t *out, int cap);
int dabhip_synth_packet_group(const dabhip_synth_cfg *cfg, int slot, int address, int n, uint8_t *out, int cap);
/* Truth of a ts_slots slot, straight from the generator (not through dabhip_ts): code word n (any sign), 188 TS bytes and 16 parity bytes,
 * before the interleaver.  Returns 204, <0 on error. */
int dabhip_synth_ts_word(const dabhip_synth_cfg *cfg, int slot, int64_t n, uint8_t *out204);
/* Device-side modulator (needs a GPU): the ensembles cfgs[0..nstreams) modulated on `device`
 * straight into DEVICE buffers iq[i] of dabhip_synth_bytes(&cfgs[i], ntf) bytes each.  The bit content comes from the
 * same generator as dabhip_synth_generate; samples may differ from the host generator's by one LSB where fp32 and
 * fp64 round apart, and the AWGN uses the same keyed generator.  Returns 0, <0 on error. */
int dabhip_synth_generate_device(const dabhip_synth_cfg *cfgs, int nstreams, int ntf, uint8_t *const *iq, int device);

#ifdef __cplusplus
}
#endif
#endif
