"""dabtools_amd — Python host side over libdabhip.so (the C ABI of include/dabhip.h).

The product is the shared library; this module is plumbing: it loads the library, declares
the C signatures and offers thin numpy-facing wrappers whose names follow the reference
(`sdr_demod`, `dab_process_frame`, `viterbi`, ...).  There is NO CPU fallback: if the
library is missing, or no MI355X is visible when a decode entry point is used, the call
raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DABHIP_LIB") or os.path.join(_HERE, "libdabhip.so")   # override: experiments with another build

STREAM_MUX_OVERFLOW, STREAM_SUBCH_OUTSIDE_CIF, STREAM_EEP_OPTION, STREAM_SUBCH_SIZE = 1, 2, 4, 8
TF_BYTES = 393216
CHUNK_BYTES = 262144
TAIL_BYTES = 1536      # the last bytes of sdr->buffer, kept as bytes beside the views (csrc/device_types.hpp: kTailBytes)
FIC_BITS = 9216
MSC_BITS = 221184
ETI_BYTES = 6144

u8p = C.POINTER(C.c_uint8)

# Viterbi decoder forms (dabhip.h: DABHIP_FORM_*): value = bit of the decoder_forms() report
FORM_AUTO, FORM_WAVE, FORM_LANE, FORM_TWO, FORM_TWO_PLAIN, FORM_FOUR = -1, 0, 1, 2, 3, 4
FORMS = {"auto": FORM_AUTO, "wave": FORM_WAVE, "lane": FORM_LANE, "two": FORM_TWO, "two-plain": FORM_TWO_PLAIN, "four": FORM_FOUR}


class DabhipError(RuntimeError):
    pass


class SubChCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("id", "start_cu", "slform", "uep_index", "eep_protlev", "size_cu")]


class ReconfCfg(C.Structure):
    _fields_ = [("at_cif", C.c_int32), ("fic_lead", C.c_int32), ("nsub", C.c_int32), ("pad", C.c_int32), ("sub", SubChCfg * 64)]


class ChannelCfg(C.Structure):
    _fields_ = [("sro_ppm", C.c_double), ("echo_delay", C.c_int32 * 2), ("echo_gain", C.c_double * 2), ("echo_phase", C.c_double * 2),
                ("echo_doppler_hz", C.c_double * 2), ("fade_depth", C.c_double), ("fade_hz", C.c_double),
                ("iq_gain_db", C.c_double), ("iq_phase_deg", C.c_double)]


class TiiCfg(C.Structure):
    """dabhip_tii_cfg: one comb of the modulator's null symbol; level_db relative to a data carrier."""
    _fields_ = [("enabled", C.c_int32), ("main_id", C.c_int32), ("sub_id", C.c_int32), ("pad", C.c_int32), ("level_db", C.c_double)]


class SynthCfg(C.Structure):
    _fields_ = [("eid", C.c_uint32), ("nsub", C.c_int32), ("sub", SubChCfg * 64), ("seed", C.c_uint64),
                ("cif_count0", C.c_int32), ("skip_samples", C.c_int32), ("amplitude", C.c_double),
                ("snr_db", C.c_double), ("cfo_hz", C.c_double),
                ("fib_patch_len", C.c_int32), ("fib_patch_from_cif", C.c_int32), ("fib_patch", C.c_uint8 * 32),
                ("reconf", ReconfCfg * 2), ("channel", ChannelCfg), ("dabplus_slots", C.c_uint64), ("dabplus_phase", C.c_int32),
                ("tii_phase", C.c_int32), ("tii", TiiCfg * 4),
                ("packet_slots", C.c_uint64), ("packet_fec_slots", C.c_uint64), ("packet_phase", C.c_int32), ("packet_pad", C.c_int32),
                ("ts_slots", C.c_uint64), ("ts_phase", C.c_int32), ("ts_pad", C.c_int32),
                ("si_mode", C.c_int32), ("si_pad", C.c_int32)]

    def set_tii(self, combs, phase=0):
        """The null symbol of every TF with (tf + phase) even carries these combs: up to four (main_id, sub_id, level_db); none = off."""
        combs = list(combs)
        if len(combs) > 4:
            raise DabhipError("set_tii: at most four combs")
        self.tii_phase = phase
        for i in range(4):
            t = self.tii[i]
            t.enabled, t.main_id, t.sub_id, t.level_db = (1,) + tuple(combs[i]) if i < len(combs) else (0, 0, 0, 0.0)

    def set_reconf(self, k, at_cif, subs, fic_lead=0):
        """Reconfiguration k (0 / 1): from logical CIF at_cif on the multiplex is `subs`, a list of (id, start_cu, slform, uep_index, eep_protlev,
        size_cu); the FIC announces it fic_lead CIFs earlier."""
        r = self.reconf[k]
        r.at_cif, r.fic_lead, r.nsub = at_cif, fic_lead, len(subs)
        for i, t in enumerate(subs):
            r.sub[i].id, r.sub[i].start_cu, r.sub[i].slform, r.sub[i].uep_index, r.sub[i].eep_protlev, r.sub[i].size_cu = t

    def multiplex(self):
        """The initial multiplex as the tuples set_reconf takes."""
        return [(s.id, s.start_cu, s.slform, s.uep_index, s.eep_protlev, s.size_cu) for s in self.sub[: self.nsub]]

    def set_fib_patch(self, data, from_cif=0):
        """Third FIB of every CIF from `from_cif` on = these bytes (<= 30) under a valid CRC: hostile / non-standard FIGs for tests."""
        data = bytes(data)[:30]
        self.fib_patch_len, self.fib_patch_from_cif = len(data), from_cif
        for i, b in enumerate(data):
            self.fib_patch[i] = b


ETI_CALLBACK = C.CFUNCTYPE(None, u8p)

_SIGNATURES = {
    "dabhip_last_error": (C.c_char_p, []),
    "dabhip_device_count": (C.c_int, []),
    "dabhip_device_identity": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int]),
    "dabhip_create_viterbi": (C.c_void_p, [C.c_int]),
    "dabhip_init_viterbi": (C.c_int, []),
    "dabhip_viterbi": (None, [C.c_void_p, u8p, u8p, C.c_int]),
    "dabhip_viterbi_batch": (C.c_int, [C.c_void_p, u8p, u8p, C.c_int, C.c_int]),
    "dabhip_sdr_init": (C.c_void_p, [C.c_int]),
    "dabhip_sdr_free": (None, [C.c_void_p]),
    "dabhip_sdr_demod": (C.c_int, [C.c_void_p, u8p, C.c_int, u8p, u8p]),
    "dabhip_sdr_coarse_timeshift": (C.c_int32, [C.c_void_p]),
    "dabhip_sdr_fine_timeshift": (C.c_int32, [C.c_void_p]),
    "dabhip_sdr_coarse_freq_shift": (C.c_int32, [C.c_void_p]),
    "dabhip_sdr_fine_freq_shift": (C.c_double, [C.c_void_p]),
    "dabhip_dab_init": (C.c_void_p, [C.c_int, ETI_CALLBACK]),
    "dabhip_dab_free": (None, [C.c_void_p]),
    "dabhip_dab_tf_fic": (u8p, [C.c_void_p]),
    "dabhip_dab_tf_msc": (u8p, [C.c_void_p]),
    "dabhip_dab_process_frame": (C.c_int, [C.c_void_p]),
    "dabhip_dab_locked": (C.c_int, [C.c_void_p]),
    "dabhip_dab_last_fibs": (C.c_int, [C.c_void_p, u8p, u8p]),
    "dabhip_engine_create": (C.c_void_p, [C.c_int]),
    "dabhip_engine_create_ex": (C.c_void_p, [C.c_int, C.c_int]),
    "dabhip_engine_destroy": (None, [C.c_void_p]),
    "dabhip_multi_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int]),
    "dabhip_multi_destroy": (None, [C.c_void_p]),
    "dabhip_multi_slices": (C.c_int, [C.c_void_p]),
    "dabhip_multi_slice_of": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "dabhip_multi_decode": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int]),
    "dabhip_multi_eti_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_multi_eti_read": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_multi_eti_drain": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dabhip_multi_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int]),
    "dabhip_multi_engine": (C.c_void_p, [C.c_void_p, C.c_int]),
    "dabhip_multi_wall_ms": (C.c_float, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_afc": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_soft": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_soft_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_parity_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_set_subchannels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_engine_decode": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int]),
    "dabhip_engine_eti_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_engine_eti_read": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_engine_eti_drain": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dabhip_engine_eti_device_ptr": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_int64)]),
    "dabhip_engine_set_afc": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_set_soft": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_set_soft_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int]),
    "dabhip_engine_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_engine_fft_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "dabhip_engine_fft_roofline": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "dabhip_stage_ofdm_fft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "dabhip_stage_demap": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, u8p, u8p]),
    "dabhip_stage_fic_decode": (C.c_int, [C.c_void_p, u8p, C.c_int, u8p, u8p]),
    "dabhip_host_parse_fibs": (C.c_int, [u8p, u8p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dabhip_host_eti_header": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), u8p, C.c_int]),
    "dabhip_host_control_replay": (C.c_int, [u8p, u8p, C.c_int, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_host_control_replay_log": (C.c_int64, [C.c_char_p, C.c_int64]),
    "dabhip_engine_stream_log": (C.c_int64, [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]),
    "dabhip_stream_log": (C.c_int64, [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]),
    "dabhip_multi_stream_log": (C.c_int64, [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]),
    "dabhip_multi_stream_log_of": (C.c_int64, [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]),
    "dabhip_dab_take_log": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    "dabhip_stream_create_on_cpus": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_multi_stream_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.c_int]),
    "dabhip_multi_stream_destroy": (None, [C.c_void_p]),
    "dabhip_multi_stream_slices": (C.c_int, [C.c_void_p]),
    "dabhip_multi_stream_streams": (C.c_int, [C.c_void_p]),
    "dabhip_multi_stream_slice_of": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dabhip_multi_stream_session": (C.c_void_p, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_prefetch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_multi_stream_feed": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_multi_stream_feed_resident": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dabhip_multi_stream_need_from": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_eti_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_status_of": (C.c_uint32, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_eti_read": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_multi_stream_eti_drain": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dabhip_multi_stream_eti_fetch": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
    "dabhip_multi_stream_eti_fetch_wait": (C.c_int, [C.c_void_p]),
    "dabhip_multi_stream_set_afc": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_set_soft": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_set_soft_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_set_parity_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_set_sync_speculation": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_set_subchannels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_host_table": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_host_fifo_new": (C.c_void_p, []),
    "dabhip_host_fifo_free": (None, [C.c_void_p]),
    "dabhip_host_fifo_call": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, u8p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int32), u8p]),
    "dabhip_host_fifo_skip_unshifted": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dabhip_synth_preset": (C.c_int, [C.c_int, C.POINTER(SynthCfg)]),
    "dabhip_synth_bytes": (C.c_size_t, [C.POINTER(SynthCfg), C.c_int]),
    "dabhip_synth_generate": (C.c_int64, [C.POINTER(SynthCfg), C.c_int, u8p, C.c_size_t]),
    "dabhip_synth_payload": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int, u8p, C.c_int]),
    "dabhip_synth_fibs": (C.c_int, [C.POINTER(SynthCfg), C.c_int, u8p]),
    "dabhip_synth_dabplus_superframe": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int, u8p, C.c_int]),
    "dabhip_synth_packet_addresses": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.POINTER(C.c_int32)]),
    "dabhip_synth_packet_cells": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int64, C.c_int, u8p, C.c_int]),
    "dabhip_synth_packet_group": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int, C.c_int, u8p, C.c_int]),
    "dabhip_dabplus_create": (C.c_void_p, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_dabplus_destroy": (None, [C.c_void_p]),
    "dabhip_dabplus_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_dabplus_superframes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "dabhip_dabplus_data": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int64]),
    "dabhip_dabplus_au_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int64]),
    "dabhip_dabplus_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_dabplus_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_synth_ts_word": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int64, u8p]),
    "dabhip_ts_create": (C.c_void_p, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_ts_destroy": (None, [C.c_void_p]),
    "dabhip_ts_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_ts_records": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "dabhip_ts_data": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int64]),
    "dabhip_ts_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_ts_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_dir_create": (C.c_void_p, [C.c_int, C.c_int]),
    "dabhip_dir_destroy": (None, [C.c_void_p]),
    "dabhip_dir_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_dir_ensemble": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "dabhip_dir_subchannels": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dabhip_dir_services": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dabhip_dir_packet_components": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dabhip_dir_complete": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_dir_resolve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p]),
    "dabhip_dir_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_dir_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_dir_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_edi_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "dabhip_edi_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "dabhip_edi_destroy": (None, [C.c_void_p]),
    "dabhip_edi_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_edi_records": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "dabhip_edi_data": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_edi_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_edi_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_edi_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_edirx_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int]),
    "dabhip_edirx_destroy": (None, [C.c_void_p]),
    "dabhip_edirx_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int]),
    "dabhip_edirx_flush": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_edirx_records": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "dabhip_edirx_frames": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_edirx_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_edirx_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_edirx_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_packet_create": (C.c_void_p, [C.c_int, C.c_int, C.POINTER(C.c_int32), u8p, C.c_int]),
    "dabhip_packet_destroy": (None, [C.c_void_p]),
    "dabhip_packet_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_packet_records": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "dabhip_packet_data": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int64]),
    "dabhip_packet_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_packet_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_packet_groups_create": (C.c_void_p, []),
    "dabhip_packet_groups_destroy": (None, [C.c_void_p]),
    "dabhip_packet_groups_push": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64, u8p, C.c_int64]),
    "dabhip_packet_groups_get": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, u8p, C.c_int64]),
    "dabhip_packet_groups_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "dabhip_engine_set_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_set_sync_speculation": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_set_sync_speculation": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_set_parity_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_parity_guard_level": (C.c_int, [C.c_void_p]),
    "dabhip_parity_guard_default_level": (C.c_int, []),
    "dabhip_parity_guard_constants": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dabhip_parity_guard_bin_scale": (C.c_double, [C.c_int]),
    "dabhip_engine_guard_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dabhip_engine_guard_overflows": (C.c_int, [C.c_void_p]),
    "dabhip_engine_set_guard_list_cap": (C.c_int, [C.c_void_p, C.c_uint32]),
    "dabhip_engine_set_launch_limits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_engine_launch_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_engine_msc_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int64)]),
    "dabhip_host_stream_state_bytes": (C.c_int, []),
    "dabhip_dab_set_launch_limits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_dab_launch_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_stream_set_launch_limits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_stream_launch_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_stream_set_parity_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stage_decision_audit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "dabhip_stage_decision_audit_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "dabhip_engine_set_subchannels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_stream_set_subchannels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_stream_create": (C.c_void_p, [C.c_int, C.c_int]),
    "dabhip_stream_destroy": (None, [C.c_void_p]),
    "dabhip_stream_feed": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_stream_prefetch": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_stream_eti_count": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_stream_eti_read": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_int64]),
    "dabhip_stream_eti_drain": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dabhip_stream_set_afc": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_set_soft": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_set_soft_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_ceiling": (C.c_int, [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "dabhip_device_alloc": (C.c_void_p, [C.c_size_t, C.c_int]),
    "dabhip_device_free": (None, [C.c_void_p]),
    "dabhip_device_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "dabhip_host_alloc": (C.c_void_p, [C.c_size_t]),
    "dabhip_host_free": (None, [C.c_void_p]),
    "dabhip_synth_generate_device": (C.c_int, [C.POINTER(SynthCfg), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int]),
    "dabhip_dab_set_soft": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_dab_set_soft_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_dab_set_decoder_forms": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dabhip_dab_decoder_forms": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dabhip_engine_set_decoder_forms": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dabhip_engine_decoder_forms": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dabhip_engine_trace_nco": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_multi_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dabhip_multi_slice_cpus": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "dabhip_engine_create_on_cpus": (C.c_void_p, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_engine_host_cpus": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "dabhip_host_placement_plan": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "dabhip_host_cpu_budget": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dabhip_engine_stream_status": (C.c_uint32, [C.c_void_p, C.c_int]),
    "dabhip_multi_stream_status": (C.c_uint32, [C.c_void_p, C.c_int]),
    "dabhip_stream_status": (C.c_uint32, [C.c_void_p, C.c_int]),
    "dabhip_stream_feed_resident": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dabhip_stream_need_from": (C.c_int64, [C.c_void_p, C.c_int]),
    "dabhip_stream_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_dab_status": (C.c_uint32, [C.c_void_p]),
    "dabhip_engine_eti_fetch": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
    "dabhip_engine_eti_fetch_wait": (C.c_int, [C.c_void_p]),
    "dabhip_stream_eti_fetch": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
    "dabhip_stream_eti_fetch_wait": (C.c_int, [C.c_void_p]),
    "dabhip_engine_demapped_tf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int8), C.POINTER(C.c_int8)]),
    "dabhip_engine_set_demod_all": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_msc_deferred": (C.c_int, [C.c_void_p]),
    "dabhip_stream_set_demod_all": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_msc_deferred": (C.c_int, [C.c_void_p]),
    "dabhip_host_lockin_deferred": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "dabhip_ingest_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint32]),
    "dabhip_ingest_destroy": (None, [C.c_void_p]),
    "dabhip_ingest_push": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_ingest_output": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dabhip_ingest_read": (C.c_int64, [C.c_void_p, C.c_int, u8p, C.c_size_t]),
    "dabhip_ingest_gain": (C.c_uint32, [C.c_void_p, C.c_int]),
    "dabhip_ingest_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_ingest_skip": (C.c_int, [C.c_void_p, C.c_int64]),
    "dabhip_ingest_taps": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int16), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dabhip_ingest_plan": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dabhip_ingest_auto_gain": (C.c_uint32, [C.c_uint64]),
    "dabhip_ingest_create_tuned": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint32, C.POINTER(C.c_int64), C.c_int]),
    "dabhip_ingest_tune_taps": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int16), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dabhip_ingest_tune_nco": (C.c_int, [C.POINTER(C.c_int16), C.c_int]),
    "dabhip_ingest_tune_step": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]),
    "dabhip_ingest_tune_plan": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dabhip_scan_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int]),
    "dabhip_scan_destroy": (None, [C.c_void_p]),
    "dabhip_scan_push": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "dabhip_scan_spectrum": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "dabhip_scan_blocks": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int]),
    "dabhip_scan_stage_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    "dabhip_scan_detect": (C.c_int, [C.POINTER(C.c_uint64), C.c_int64, C.c_int64, C.c_void_p, C.c_int]),
    "dabhip_scan_plan": (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dabhip_engine_set_tii": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_engine_tii_sums": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "dabhip_engine_tii": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dabhip_engine_tii_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "dabhip_stream_set_tii": (C.c_int, [C.c_void_p, C.c_int]),
    "dabhip_stream_tii_sums": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "dabhip_stream_tii": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "dabhip_stream_tii_reset": (C.c_int, [C.c_void_p]),
    "dabhip_tii_detect": (C.c_int, [C.POINTER(C.c_uint64), C.c_void_p, C.c_int]),
    "dabhip_tii_carriers": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int16), C.c_int]),
    "dabhip_stage_tii": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]),
}

_lib = None


def build_library(force=False):
    """Compile dabtools_amd/csrc into dabtools_amd/libdabhip.so (hipcc, gfx950)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j8"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """The loaded libdabhip.so.  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DabhipError("libdabhip.so is missing (%s): run __graft_entry__.build() / make -C dabtools_amd/csrc" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(L, name)   # AttributeError here = header/library mismatch
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def last_error():
    return (lib().dabhip_last_error() or b"").decode()


def _p(a):
    return a.ctypes.data_as(u8p)


def _form(f):
    """A form given by name ("wave", "lane", "two", "two-plain", "four", "auto"), None (= auto) or by its number."""
    if f is None:
        return FORM_AUTO
    return FORMS[f] if isinstance(f, str) else int(f)


def _form_names(mask):
    return {name for name, v in FORMS.items() if v >= 0 and mask >> v & 1}


def _decoder_forms(fn, h):
    m, f = C.c_uint32(0), C.c_uint32(0)
    _need(fn(h, C.byref(m), C.byref(f)) == 0, "decoder_forms")
    return m.value, f.value


# launch limits (dabhip.h: DABHIP_LIMIT_*) and the launch report (DABHIP_REPORT_*), in the C ABI's order
LAUNCH_LIMITS = ("decision_rows", "regroup_tiles", "fic_group_tiles", "gather_descs", "fetch_words", "fft_chunk_tfs")
LAUNCH_REPORT = ("decoder", "regroup", "fic_group", "gather", "ofdm_chunks", "fic_prepass", "fetch_form", "fetches", "gather_calls", "decoder_planned")
FETCH_NONE, FETCH_KERNEL, FETCH_COPY_ENGINE = 0, 1, 2


def _set_launch_limits(fn, h, limits):
    unknown = set(limits) - set(LAUNCH_LIMITS)
    if unknown:
        raise ValueError("no such launch limit: %s" % ", ".join(sorted(unknown)))
    arr = (C.c_int64 * len(LAUNCH_LIMITS))(*[int(limits.get(k, 0)) for k in LAUNCH_LIMITS])
    _need(fn(h, arr, len(LAUNCH_LIMITS)) == 0, "set_launch_limits")


def _launch_report(fn, h):
    out = (C.c_int64 * len(LAUNCH_REPORT))()
    _need(fn(h, out, len(LAUNCH_REPORT)) == len(LAUNCH_REPORT), "launch_report")
    return dict(zip(LAUNCH_REPORT, list(out)))


def _need(cond, what):
    if not cond:
        raise DabhipError("%s: %s" % (what, last_error()))


def device_identity(device):
    """(PCI bus id, name) of a device index (dabhip_device_identity)."""
    bus, name = C.create_string_buffer(64), C.create_string_buffer(256)
    _need(lib().dabhip_device_identity(int(device), bus, len(bus), name, len(name)) == 0, "device_identity")
    return bus.value.decode(), name.value.decode()


def _guard_level(level):
    """False / 0 -> off, True -> the library's default level (-1), 1 / 2 -> that level (dabhip.h: DABHIP_GUARD_*)."""
    if level is True:
        return -1
    if level is False or level is None:
        return 0
    return int(level)


def guard_constants(level):
    """(bound on a bin's error relative to |x|_2, bound on the product's rounding relative to |cur|_1 |prev|_1) of guard level 1 or 2."""
    a, b = C.c_double(0), C.c_double(0)
    _need(lib().dabhip_parity_guard_constants(int(level), C.byref(a), C.byref(b)) == 0, "parity_guard_constants")
    return a.value, b.value


def guard_bin_scale(raw_bin):
    """Fraction of the proven level's bin constant that bounds raw bin k's error (dabhip_parity_guard_bin_scale)."""
    return lib().dabhip_parity_guard_bin_scale(int(raw_bin))


def guard_default_level():
    return lib().dabhip_parity_guard_default_level()


# ---- synthetic modulator --------------------------------------------------------------------
def synth_preset(preset=0, seed=1, cif_count0=0, skip_samples=0, snr_db=1000.0, amplitude=1.0, cfo_hz=0.0):
    cfg = SynthCfg()
    _need(lib().dabhip_synth_preset(preset, C.byref(cfg)) == 0, "synth_preset")
    cfg.seed = seed
    cfg.cif_count0 = cif_count0
    cfg.skip_samples = skip_samples
    cfg.snr_db = snr_db
    cfg.amplitude = amplitude
    cfg.cfo_hz = cfo_hz
    return cfg


def synth_generate(cfg, ntf):
    n = lib().dabhip_synth_bytes(C.byref(cfg), ntf)
    iq = np.empty(n, dtype=np.uint8)
    got = lib().dabhip_synth_generate(C.byref(cfg), ntf, _p(iq), n)
    if cfg.channel.sro_ppm != 0.0:             # the resampler decides the count; n is the capacity
        _need(0 < got <= n, "synth_generate")
        return iq[:got].copy()
    _need(got == n, "synth_generate")
    return iq


def synth_bytes(cfg, ntf):
    return lib().dabhip_synth_bytes(C.byref(cfg), ntf)


def synth_generate_device(cfgs, ntf, ptrs, device=0):
    """Modulate the ensembles cfgs on the GPU into the device buffers at ptrs (ints; synth_bytes(cfg, ntf) bytes each)."""
    arr = (SynthCfg * len(cfgs))(*cfgs)
    p = (C.c_void_p * len(ptrs))(*ptrs)
    _need(lib().dabhip_synth_generate_device(arr, len(cfgs), ntf, p, device) == 0, "synth_generate_device")


def synth_payload(cfg, cif_index, slot):
    buf = np.zeros(ETI_BYTES, dtype=np.uint8)          # a sub-channel's bytes per CIF lie inside one ETI frame (EEP 4-B at n = 57: 5472)
    n = lib().dabhip_synth_payload(C.byref(cfg), cif_index, slot, _p(buf), buf.size)
    _need(n >= 0, "synth_payload")
    return buf[:n].copy()


def synth_fibs(cfg, cif_index):
    buf = np.zeros(96, dtype=np.uint8)
    _need(lib().dabhip_synth_fibs(C.byref(cfg), cif_index, _p(buf)) == 96, "synth_fibs")
    return buf


def synth_dabplus_superframe(cfg, sf_index, slot):
    """The unprotected 110 s bytes of DAB+ superframe sf_index of a dabplus_slots slot (before RS parity and interleaving)."""
    buf = np.zeros(110 * 72, dtype=np.uint8)
    n = lib().dabhip_synth_dabplus_superframe(C.byref(cfg), sf_index, slot, _p(buf), buf.size)
    _need(n >= 0, "synth_dabplus_superframe")
    return buf[:n].copy()


def synth_packet_addresses(cfg, slot):
    """The addresses the data groups of a packet_slots slot go out on (two or three)."""
    a = (C.c_int32 * 3)()
    n = lib().dabhip_synth_packet_addresses(C.byref(cfg), slot, a)
    _need(n >= 0, "synth_packet_addresses")
    return [int(a[i]) for i in range(n)]


def synth_packet_cells(cfg, slot, cell_index, ncells):
    """ncells transmitted cells of a packet_slots slot from cell_index on (cells counted from logical CIF 0's first): an (ncells, 24) array."""
    buf = np.zeros((ncells, 24), dtype=np.uint8)
    _need(lib().dabhip_synth_packet_cells(C.byref(cfg), slot, cell_index, ncells, _p(buf), buf.size) == buf.size, "synth_packet_cells")
    return buf


def synth_ts_word(cfg, slot, n):
    """Code word n (any sign) of a ts_slots slot before the interleaver: 188 TS bytes and 16 parity bytes."""
    buf = np.zeros(204, dtype=np.uint8)
    _need(lib().dabhip_synth_ts_word(C.byref(cfg), slot, int(n), _p(buf)) == 204, "synth_ts_word")
    return buf


def synth_packet_group(cfg, slot, address, n):
    """The n-th data group of an address of a packet_slots slot, counted from unit 0 on."""
    buf = np.zeros(8208, dtype=np.uint8)
    size = lib().dabhip_synth_packet_group(C.byref(cfg), slot, address, n, _p(buf), buf.size)
    _need(size >= 0, "synth_packet_group")
    return buf[:size].copy()


def stream_ceiling(device=0, nbytes=4 << 30, reps=3):
    """GB/s a bare streaming kernel reaches on this device: {"fill", "copy", "k2_mix"} (k_probe.hip)."""
    g = (C.c_double * 3)()
    _need(lib().dabhip_stream_ceiling(device, nbytes, reps, g) == 0, "stream_ceiling")
    return {"fill": g[0], "copy": g[1], "k2_mix": g[2]}


class _Handle:
    """A C handle in self._h, destroyed once by the entry named _destroy: at close() or when the object goes."""
    _h = _destroy = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:                       # at interpreter shutdown the module globals may already be gone
            self.close()
        except Exception:
            pass


def _stage_ms(fn, h, n):
    """The *_stage_ms entries of the side stages: {stage: GPU time of the last push in ms}, at most n stages."""
    names, ms = (C.c_char_p * n)(), (C.c_float * n)()
    return {names[i].decode(): ms[i] for i in range(fn(h, names, ms, n))}


def _push_samples(fn, what, h, nstreams, ptrs, sizes, on_device):
    """dabhip_ingest_push and dabhip_scan_push over raw addresses, one per stream."""
    _need(len(ptrs) == nstreams and len(sizes) == nstreams, what + ": one input per stream")
    n = fn(h, (C.c_void_p * nstreams)(*ptrs), (C.c_size_t * nstreams)(*sizes), 1 if on_device else 0)
    _need(n >= 0, what)
    return n


def _sample_bytes(what, nstreams, arrays):
    """One array per stream as bytes (the caller keeps them alive over the push)."""
    _need(len(arrays) == nstreams, what + ": one array per stream")
    return [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]


def _one_stream_counts(what, nstreams, n):
    """The counts of a push that names none: all n items are the one stream's."""
    _need(nstreams == 1, what + ": counts needed for several streams")
    return [n]


def _eti_frames_arg(what, nstreams, frames, counts):
    """The frames of a push of ETI frames (DabPlus.push has the forms) as (src, cnt, on_device, keepalive): the address, the per-stream counts
    as the C entry takes them, and for host frames the array that holds them (else None), which the caller keeps alive."""
    if isinstance(frames, tuple):
        (ptr, counts), arr = frames, None
    elif isinstance(frames, list):
        counts = [np.asarray(f).size // ETI_BYTES for f in frames]
        arr = np.ascontiguousarray(np.concatenate([np.asarray(f, dtype=np.uint8).reshape(-1) for f in frames]) if frames else np.zeros(0, np.uint8))
    else:
        arr = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        if counts is None:
            counts = _one_stream_counts(what, nstreams, arr.size // ETI_BYTES)
    cnt = (C.c_int64 * nstreams)(*[int(c) for c in counts])
    return C.c_void_p(ptr if arr is None else arr.ctypes.data), cnt, int(arr is None), arr


def _fetch(fn, what, dtype, *at):
    """The records / data entries of the stages of ETI frames: fn(*at, None, 0) says how many items there are, fn(*at, dst, n) brings them."""
    n = fn(*at, None, 0)
    _need(n >= 0, what)
    out = np.zeros(n, dtype=dtype)
    _need(fn(*at, _p(out), n) == n, what)
    return out


class HostBuffer:
    """nbytes of page-locked host memory (dabhip_host_alloc): .array is a numpy view, .ptr its address.  Uploads from it are
    plain asynchronous DMA at the PCIe rate; pageable memory goes through the engine's staging ring instead."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().dabhip_host_alloc(max(self.nbytes, 1))
        _need(self.ptr, "host_alloc")
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, u8p), (self.nbytes,))

    def free(self):
        if self.ptr:
            self.array = None
            lib().dabhip_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """nbytes of device memory (dabhip_device_alloc): .ptr for the entry points that take device pointers."""

    def __init__(self, nbytes, device=0):
        self.nbytes = int(nbytes)
        self.ptr = lib().dabhip_device_alloc(self.nbytes, device)
        _need(self.ptr, "device_alloc")

    def upload(self, array):
        a = np.ascontiguousarray(array, dtype=np.uint8)
        _need(a.size <= self.nbytes and lib().dabhip_device_copy(self.ptr, a.ctypes.data, a.size, 1) == 0, "device_copy")

    def download(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        _need(lib().dabhip_device_copy(out.ctypes.data, self.ptr, self.nbytes, 0) == 0, "device_copy")
        return out

    def free(self):
        if self.ptr:
            lib().dabhip_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- host-side control plane (no GPU needed) ----------------------------------------------------
def host_parse_fibs(fibs, crc_ok):
    fibs = np.ascontiguousarray(fibs, dtype=np.uint8)
    crc_ok = np.ascontiguousarray(crc_ok, dtype=np.uint8)
    hdr = np.zeros(3, dtype=np.int32)
    sub = np.zeros((64, 8), dtype=np.int32)
    _need(lib().dabhip_host_parse_fibs(_p(fibs), _p(crc_ok), hdr.ctypes.data_as(C.POINTER(C.c_int32)),
                                       sub.ctypes.data_as(C.POINTER(C.c_int32))) == 0, "host_parse_fibs")
    return hdr, sub


def host_eti_header(hdr, sub):
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    sub = np.ascontiguousarray(sub, dtype=np.int32)
    out = np.zeros(272, dtype=np.uint8)
    n = lib().dabhip_host_eti_header(hdr.ctypes.data_as(C.POINTER(C.c_int32)), sub.ctypes.data_as(C.POINTER(C.c_int32)), _p(out), out.size)
    _need(n > 0, "host_eti_header")
    return out[:n].copy()


def host_stream_state_bytes():
    """sizeof the front end's per-stream state (dabhip_host_stream_state_bytes)"""
    return lib().dabhip_host_stream_state_bytes()


def host_lockin_deferred(locked, okcount, ntf):
    """The lock-in rule (dabhip.h): how many of the next ntf TFs of a stream cannot be locked, given the back end's state in front of them."""
    return int(lib().dabhip_host_lockin_deferred(1 if locked else 0, int(okcount), int(ntf)))


def host_control_replay(fibs, crc_ok):
    fibs = np.ascontiguousarray(fibs, dtype=np.uint8).reshape(-1, 384)
    crc_ok = np.ascontiguousarray(crc_ok, dtype=np.uint8).reshape(-1, 12)
    ntf = fibs.shape[0]
    cap = 4 * ntf + 4
    first = np.zeros(cap, dtype=np.int32)
    hlen = np.zeros(cap, dtype=np.int32)
    hdrs = np.zeros((cap, 272), dtype=np.uint8)
    n = lib().dabhip_host_control_replay(_p(fibs), _p(crc_ok), ntf, first.ctypes.data_as(C.POINTER(C.c_int32)), _p(hdrs),
                                         hlen.ctypes.data_as(C.POINTER(C.c_int32)), cap)
    _need(n >= 0, "host_control_replay")
    return first[:n], [hdrs[i, :hlen[i]].copy() for i in range(n)]


def host_control_replay_log():
    """The operator messages (dab.c:51,57,78-82) of this thread's last host_control_replay, as text."""
    buf = C.create_string_buffer(1 << 16)
    _need(lib().dabhip_host_control_replay_log(buf, len(buf)) >= 0, "host_control_replay_log")
    return buf.value.decode("ascii")


def host_placement_plan(slice_node, node_cpulist, ncpu):
    """dabhip_host_placement_plan: cpu_slice[c] = slice CPU c is given to (-1: none), for slices on NUMA nodes slice_node[i]."""
    nodes = (C.c_int32 * len(slice_node))(*slice_node)
    lists = (C.c_char_p * len(node_cpulist))(*[s.encode() for s in node_cpulist])
    out = (C.c_int32 * ncpu)()
    n = lib().dabhip_host_placement_plan(nodes, len(slice_node), lists, len(node_cpulist), out, ncpu)
    _need(n >= 0, "host_placement_plan")
    return n, list(out)


def host_cpu_budget():
    """(usable CPUs, CPUs in the affinity mask, CFS quota in CPUs or 0) as the library sizes its host pools (csrc/placement.hpp)."""
    a, q = C.c_int(0), C.c_int(0)
    n = lib().dabhip_host_cpu_budget(C.byref(a), C.byref(q))
    return n, a.value, q.value


def host_table(which):
    """The product's constant tables (dabhip_host_table): 0 UEP profiles (64 x 11), 1 puncturing vectors (24 x 32),
    2 frequency de-interleaver (1536), 3 phase reference symbol quarter turns (1536)."""
    out = np.zeros(4096, dtype=np.int32)
    n = lib().dabhip_host_table(which, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
    _need(n > 0, "host_table")
    shape = {0: (64, 11), 1: (24, 32)}.get(which, (n,))
    return out[:n].reshape(shape)


class HostFifo(_Handle):
    """The FIFO / frame-buffer bookkeeping of the sync-scan kernel, on the host (dabhip_host_fifo_*)."""
    _destroy = "dabhip_host_fifo_free"

    def __init__(self):
        self._h = lib().dabhip_host_fifo_new()
        _need(self._h, "host_fifo_new")

    def call(self, coarse_timeshift, fine_timeshift, stream=None, chunk_bytes=CHUNK_BYTES):
        """One sdr_demod call appending chunk_bytes -> (status 0/1/2, [(seg_end, seg_src), ...], fifo_count).  stream (uint8 array holding at least
        the bytes fed so far): the last 1536 bytes of sdr->buffer are tracked as bytes and left in self.tail."""
        nseg, cnt = C.c_int32(0), C.c_int32(0)
        ends = np.zeros(12, dtype=np.int32)
        srcs = np.zeros(12, dtype=np.int64)
        self.tail = np.zeros(TAIL_BYTES, dtype=np.uint8) if stream is not None else None
        r = lib().dabhip_host_fifo_call(self._h, coarse_timeshift, fine_timeshift, chunk_bytes, _p(stream) if stream is not None else None, C.byref(nseg),
                                        ends.ctypes.data_as(C.POINTER(C.c_int32)), srcs.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cnt),
                                        _p(self.tail) if stream is not None else None)
        _need(r >= 0, "host_fifo_call")
        return r, [(int(ends[i]), int(srcs[i])) for i in range(nseg.value)], cnt.value

    def skip_unshifted(self, ncalls):
        """ncalls further 262144-byte calls without any time shift, counters only (dabhip_host_fifo_skip_unshifted) -> (fed, consumed)"""
        fed, consumed = C.c_int64(0), C.c_int64(0)
        _need(lib().dabhip_host_fifo_skip_unshifted(self._h, ncalls, C.byref(fed), C.byref(consumed)) == 0, "host_fifo_skip_unshifted")
        return fed.value, consumed.value

    @staticmethod
    def materialise(stream, view, tail=None):
        """The 393216 bytes of sdr->buffer a view (and the tail bytes kept beside it) describe."""
        buf = np.zeros(TF_BYTES, dtype=np.uint8)
        lo = 0
        for end, src in view:
            if src >= 0:
                buf[lo:end] = stream[src + lo:src + end]
            lo = end
        if tail is not None:
            buf[TF_BYTES - TAIL_BYTES:] = tail
        return buf


# ---- S1 -----------------------------------------------------------------------------------------
def viterbi(symbols, framebits, n=1):
    """Batch form of the reference's viterbi(p, symbols, data, framebits) (viterbi.h:8)."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    assert sym.size == n * 4 * (framebits + 6)
    out = np.zeros((n, framebits // 8), dtype=np.uint8)
    r = lib().dabhip_viterbi_batch(None, _p(sym), _p(out), framebits, n)
    _need(r == n, "viterbi")
    return out


# ---- S2 -----------------------------------------------------------------------------------------
class Sdr(_Handle):
    """sdr_init + sdr_demod (input_sdr.h:43-44) for one stream."""
    _destroy = "dabhip_sdr_free"

    def __init__(self, device=0):
        self._h = lib().dabhip_sdr_init(device)
        _need(self._h, "sdr_init")
        self.fic = np.zeros(FIC_BITS, dtype=np.uint8)
        self.msc = np.zeros(MSC_BITS, dtype=np.uint8)

    def demod(self, chunk):
        chunk = np.ascontiguousarray(chunk, dtype=np.uint8)
        r = lib().dabhip_sdr_demod(self._h, _p(chunk), chunk.size, _p(self.fic), _p(self.msc))
        _need(r >= 0, "sdr_demod")
        return r

    @property
    def state(self):
        L = lib()
        return (L.dabhip_sdr_coarse_timeshift(self._h), L.dabhip_sdr_fine_timeshift(self._h),
                L.dabhip_sdr_coarse_freq_shift(self._h), L.dabhip_sdr_fine_freq_shift(self._h))


# ---- S3 -----------------------------------------------------------------------------------------
class Dab(_Handle):
    """init_dab_state + dab_process_frame (dab.h:91-92) for one stream."""
    _destroy = "dabhip_dab_free"

    def __init__(self, device=0, soft=False, forms=None, soft_lanes=False):
        self.frames = []
        self._cb = ETI_CALLBACK(lambda p: self.frames.append(np.frombuffer(C.string_at(p, ETI_BYTES), np.uint8)))
        self._h = lib().dabhip_dab_init(device, self._cb)
        _need(self._h, "dab_init")
        self.fic = np.ctypeslib.as_array(lib().dabhip_dab_tf_fic(self._h), (FIC_BITS,))
        self.msc = np.ctypeslib.as_array(lib().dabhip_dab_tf_msc(self._h), (MSC_BITS,))
        if soft:       # extension: the hand-off carries signed 4-bit values (int8 views of the same arrays)
            _need(lib().dabhip_dab_set_soft(self._h, 1) == 0, "dab_set_soft")
            self.fic, self.msc = self.fic.view(np.int8), self.msc.view(np.int8)
        if soft_lanes:
            self.set_soft_lanes(True)
        if forms is not None:
            self.set_decoder_forms(*forms)

    def set_decoder_forms(self, msc=None, fic=None):
        """Force the Viterbi form of the MSC / FIC decodes (names or FORM_* numbers; None = the default rule)."""
        _need(lib().dabhip_dab_set_decoder_forms(self._h, _form(msc), _form(fic)) == 0, "dab_set_decoder_forms")

    def set_soft_lanes(self, enable):
        """see Engine.set_soft_lanes"""
        _need(lib().dabhip_dab_set_soft_lanes(self._h, 1 if enable else 0) == 0, "dab_set_soft_lanes")

    def decoder_forms(self, masks=False):
        """The forms that ran in the last process_frame: ({MSC form names}, {FIC form names}), or the two bit masks."""
        m, f = _decoder_forms(lib().dabhip_dab_decoder_forms, self._h)
        return (m, f) if masks else (_form_names(m), _form_names(f))

    def set_launch_limits(self, **limits):
        """see Engine.set_launch_limits"""
        _set_launch_limits(lib().dabhip_dab_set_launch_limits, self._h, limits)

    def launch_report(self):
        """The launches of the last process_frame (see Engine.launch_report)."""
        return _launch_report(lib().dabhip_dab_launch_report, self._h)

    def process_frame(self):
        r = lib().dabhip_dab_process_frame(self._h)
        _need(r >= 0, "dab_process_frame")
        return r

    @property
    def locked(self):
        return bool(lib().dabhip_dab_locked(self._h))

    def take_log(self):
        """What the reference's dab_process_frame would have printed on stderr since the last call (dabhip_dab_take_log)."""
        buf = C.create_string_buffer(1 << 16)
        _need(lib().dabhip_dab_take_log(self._h, buf, len(buf)) >= 0, "dab_take_log")
        return buf.value.decode("ascii")

    @property
    def status(self):
        return int(lib().dabhip_dab_status(self._h))

    def last_fibs(self):
        fibs = np.zeros((12, 32), dtype=np.uint8)
        ok = np.zeros(12, dtype=np.uint8)
        lib().dabhip_dab_last_fibs(self._h, _p(fibs), _p(ok))
        return fibs, ok


# ---- batch engine -------------------------------------------------------------------------------
# one record of dabhip_dabplus_superframes (dabhip.h: dabhip_dabplus_sf)
DABPLUS_SF = np.dtype([("stream", "<i4"), ("sub", "<i4"), ("fct", "<i4"), ("s", "<i4"), ("fire_ok", "u1"), ("layout_ok", "u1"), ("rfa", "u1"),
                       ("dac_rate", "u1"), ("sbr_flag", "u1"), ("aac_channel_mode", "u1"), ("ps_flag", "u1"), ("mpeg_surround_config", "u1"),
                       ("num_aus", "<i4"), ("au_start", "<u2", (6,)), ("au_len", "<u2", (6,)), ("crc_ok", "<u4"), ("rs_corrected", "<i4"),
                       ("rs_failed", "<i4")])
assert DABPLUS_SF.itemsize == 64
DABPLUS_STATS = ("superframes", "fire_fails", "rs_corrected_bytes", "rs_failed_codewords", "aus", "au_crc_fails", "sync_losses")


class DabPlus(_Handle):
    """DAB+ audio out of ETI frames on the GPU (dabhip_dabplus_*): superframe sync, RS(120,110) correction, AU CRCs, for nstreams streams and the
    DAB+ sub-channels subch_ids of each.  State (sync, the last 4 frames of every stream) carries from push to push."""
    _destroy = "dabhip_dabplus_destroy"

    def __init__(self, nstreams, subch_ids, device=0):
        self.nstreams, self.subch_ids = int(nstreams), [int(i) for i in subch_ids]
        ids = (C.c_int32 * len(self.subch_ids))(*self.subch_ids)
        self._h = lib().dabhip_dabplus_create(device, self.nstreams, ids, len(self.subch_ids))
        _need(self._h, "dabplus_create")

    def push(self, frames, counts=None):
        """frames: a list of per-stream arrays of ETI frames (n x 6144 bytes each), one array of all frames stream after stream with counts, or
        (device_ptr, counts) for frames in device memory (Engine.eti_device_ptr's layout).  Returns the superframes this push completed."""
        src, cnt, on_dev, keep = _eti_frames_arg("dabplus_push", self.nstreams, frames, counts)
        if keep is not None:
            self._keep = keep
        n = lib().dabhip_dabplus_push(self._h, src, cnt, on_dev)
        _need(n >= 0, "dabplus_push")
        return n

    def superframes(self, stream=0, sub=0):
        """Records of the last push's superframes of (stream, sub-channel index): a DABPLUS_SF array."""
        return _fetch(lib().dabhip_dabplus_superframes, "dabplus_superframes", DABPLUS_SF, self._h, stream, sub)

    def data(self, stream=0, sub=0):
        """The corrected 110 s audio bytes of those superframes, one after another."""
        return _fetch(lib().dabhip_dabplus_data, "dabplus_data", np.uint8, self._h, stream, sub)

    def au_bytes(self, stream=0, sub=0):
        """The AUs of the last push with a good CRC, CRC bytes stripped, one after another."""
        return _fetch(lib().dabhip_dabplus_au_bytes, "dabplus_au_bytes", np.uint8, self._h, stream, sub)

    def aus(self, stream=0, sub=0):
        """The same AUs as a list of uint8 arrays, in order."""
        blob, out, off = self.au_bytes(stream, sub), [], 0
        for r in self.superframes(stream, sub):
            if not r["layout_ok"]:
                continue
            for k in range(r["num_aus"]):
                if r["crc_ok"] >> k & 1:
                    n = int(r["au_len"][k]) - 2
                    out.append(blob[off:off + n])
                    off += n
        return out

    def stats(self, stream=0, sub=0):
        """Counters since creation, in DABPLUS_STATS order (int64 array of 7)."""
        c = np.zeros(7, dtype=np.int64)
        _need(lib().dabhip_dabplus_stats(self._h, stream, sub, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "dabplus_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push per stage: {"locate", "sync", "rs", "au", "carry"} in ms."""
        return _stage_ms(lib().dabhip_dabplus_stage_ms, self._h, 5)


# ---- packet-mode data (dabhip.h: dabhip_packet_*, dabhip_packet_groups_*) --------------------------------------------
# one record of dabhip_packet_records (dabhip_packet_rec) and of dabhip_packet_groups_get (dabhip_packet_group)
PACKET_REC = np.dtype([("cell", "<i8"), ("address", "<u2"), ("length", "u1"), ("continuity", "u1"), ("first_last", "u1"), ("command", "u1"),
                       ("useful_length", "u1"), ("flags", "u1")])
assert PACKET_REC.itemsize == 16
PACKET_GROUP = np.dtype([("address", "<i4"), ("length", "<i4"), ("ext_flag", "u1"), ("crc_flag", "u1"), ("seg_flag", "u1"), ("ua_flag", "u1"),
                         ("type", "u1"), ("continuity", "u1"), ("repetition", "u1"), ("crc_ok", "u1"), ("ext_field", "<u2"), ("last_segment", "u1"),
                         ("header_ok", "u1"), ("segment_number", "<i4"), ("transport_id", "<i4")])
assert PACKET_GROUP.itemsize == 28
PACKET_FROM_FEC, PACKET_FROM_MISS = 1, 2
PACKET_STATS = ("units", "missed_frames", "sync_losses", "cells_skipped", "bad_cells", "packets", "rs_corrected_bytes", "rs_failed_codewords")
PACKET_GROUP_STATS = ("groups", "dropped", "orphan_packets", "crc_fails")


class Packet(_Handle):
    """Packet-mode data out of ETI frames on the GPU (dabhip_packet_*): cell streams, FEC frame sync and RS(204,188) correction where fec is set,
    packet CRCs, for nstreams streams and the sub-channels subch_ids of each.  State (sync, at most 102 cells per lane) carries from push to push."""
    _destroy = "dabhip_packet_destroy"

    def __init__(self, nstreams, subch_ids, fec=None, device=0):
        self.nstreams, self.subch_ids = int(nstreams), [int(i) for i in subch_ids]
        self.fec = [1 if f else 0 for f in (fec if fec is not None else [0] * len(self.subch_ids))]
        _need(len(self.fec) == len(self.subch_ids), "packet_create: one FEC flag per sub-channel")
        ids = (C.c_int32 * len(self.subch_ids))(*self.subch_ids)
        flags = np.array(self.fec + [0], dtype=np.uint8)
        self._h = lib().dabhip_packet_create(device, self.nstreams, ids, _p(flags), len(self.subch_ids))
        _need(self._h, "packet_create")

    def push(self, frames, counts=None):
        """frames as DabPlus.push takes them.  Returns the packets this push took."""
        src, cnt, on_dev, keep = _eti_frames_arg("packet_push", self.nstreams, frames, counts)
        if keep is not None:
            self._keep = keep
        n = lib().dabhip_packet_push(self._h, src, cnt, on_dev)
        _need(n >= 0, "packet_push")
        return n

    def records(self, stream=0, sub=0):
        """Records of the last push's packets of (stream, sub-channel index): a PACKET_REC array."""
        return _fetch(lib().dabhip_packet_records, "packet_records", PACKET_REC, self._h, stream, sub)

    def data(self, stream=0, sub=0):
        """The useful bytes of those packets, one after another."""
        return _fetch(lib().dabhip_packet_data, "packet_data", np.uint8, self._h, stream, sub)

    def stats(self, stream=0, sub=0):
        """Counters since creation, in PACKET_STATS order (int64 array of 8)."""
        c = np.zeros(8, dtype=np.int64)
        _need(lib().dabhip_packet_stats(self._h, stream, sub, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "packet_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push per stage: {"locate", "sync", "gather", "rs", "cand", "walk", "carry"} in ms."""
        return _stage_ms(lib().dabhip_packet_stage_ms, self._h, 7)


# ---- MPEG-2 transport stream (dabhip.h: dabhip_ts_*) ------------------------------------------------------------------
TS_REC = np.dtype([("pos", "<i8"), ("pid", "<u2"), ("continuity", "u1"), ("flags", "u1"), ("corrected", "u1"), ("pad", "u1", (3,))])
assert TS_REC.itemsize == 16
TS_FROM_MISS, TS_RS_FAILED, TS_TEI, TS_PUSI, TS_BAD_SYNC = 1, 2, 4, 8, 16
TS_STATS = ("packets", "from_missed_slots", "sync_losses", "bytes_skipped", "rs_corrected_bytes", "rs_failed_words", "bad_sync_packets", "null_packets")
TS_STAGES = ("locate", "runs", "sync", "jobs", "gather", "syndrome", "decode", "parse", "carry")


class Ts(_Handle):
    """MPEG-2 TS packets out of ETI frames on the GPU (dabhip_ts_*): slot sync on the 0x47 bytes, the byte de-interleaver and RS(204,188), for
    nstreams streams and the sub-channels subch_ids of each.  State (sync, at most 2447 bytes per lane) carries from push to push."""
    _destroy = "dabhip_ts_destroy"

    def __init__(self, nstreams, subch_ids, device=0):
        self.nstreams, self.subch_ids = int(nstreams), [int(i) for i in subch_ids]
        ids = (C.c_int32 * len(self.subch_ids))(*self.subch_ids)
        self._h = lib().dabhip_ts_create(device, self.nstreams, ids, len(self.subch_ids))
        _need(self._h, "ts_create")

    def push(self, frames, counts=None):
        """frames as Packet.push takes them.  Returns the packets of this push."""
        src, cnt, on_dev, keep = _eti_frames_arg("ts_push", self.nstreams, frames, counts)
        if keep is not None:
            self._keep = keep
        n = lib().dabhip_ts_push(self._h, src, cnt, on_dev)
        _need(n >= 0, "ts_push")
        return n

    def records(self, stream=0, sub=0):
        """Records of the last push's packets of (stream, sub-channel index): a TS_REC array."""
        return _fetch(lib().dabhip_ts_records, "ts_records", TS_REC, self._h, stream, sub)

    def data(self, stream=0, sub=0):
        """Their bytes: an (n, 188) array, failed words as received."""
        return _fetch(lib().dabhip_ts_data, "ts_data", np.uint8, self._h, stream, sub).reshape(-1, 188)

    def stats(self, stream=0, sub=0):
        """Counters since creation, in TS_STATS order (int64 array of 8)."""
        c = np.zeros(8, dtype=np.int64)
        _need(lib().dabhip_ts_stats(self._h, stream, sub, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "ts_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push per stage: TS_STAGES in ms."""
        return _stage_ms(lib().dabhip_ts_stage_ms, self._h, len(TS_STAGES))


# ---- ensemble directory (dabhip.h: dabhip_dir_*) --------------------------------------------------------------------------
_DIR_META = [("first_frame", "<i8"), ("last_frame", "<i8"), ("changes", "<i8")]
DIR_ENSEMBLE = np.dtype([("have", "u1"), ("charset", "u1"), ("eid", "<u2"), ("label_eid", "<u2"), ("char_flags", "<u2"), ("label", "u1", (16,)),
                         ("change_flag", "u1"), ("al", "u1"), ("cif_hi", "u1"), ("cif_lo", "u1"), ("lto", "u1"), ("ecc", "u1"), ("inter_table", "u1"),
                         ("utc_flag", "u1"), ("mjd", "<u4"), ("lsi", "u1"), ("hours", "u1"), ("minutes", "u1"), ("seconds", "u1"), ("milliseconds", "<u2"),
                         ("pad", "u1", (6,)), ("time_frame", "<i8")] + _DIR_META)
DIR_SUBCH = np.dtype([("have", "u1"), ("id", "u1"), ("form", "u1"), ("uep_index", "u1"), ("protlev", "u1"), ("fec_scheme", "u1"), ("start_cu", "<u2"),
                      ("size_cu", "<u2"), ("bitrate", "<u2"), ("pad", "u1", (4,))] + _DIR_META)
DIR_SERVICE = np.dtype([("sid", "<u4"), ("pd", "u1"), ("have", "u1"), ("info", "u1"), ("ncomp", "u1"), ("comp", "u1", (30,)), ("charset", "u1"), ("pad0", "u1"),
                        ("label", "u1", (16,)), ("char_flags", "<u2"), ("pad", "u1", (6,))] + _DIR_META)
DIR_PKTCOMP = np.dtype([("scid", "<u2"), ("address", "<u2"), ("scca", "<u2"), ("subch", "u1"), ("dscty", "u1"), ("dg", "u1"), ("scca_flag", "u1"),
                        ("pad", "u1", (6,))] + _DIR_META)
DIR_TARGET = np.dtype([(n, "<i4") for n in ("kind", "subch", "address", "dg", "dscty", "fec", "scid", "primary")])
assert (DIR_ENSEMBLE.itemsize, DIR_SUBCH.itemsize, DIR_SERVICE.itemsize, DIR_PKTCOMP.itemsize, DIR_TARGET.itemsize) == (80, 40, 88, 40, 32)
DIR_KINDS = ("UNKNOWN", "MP2", "DABPLUS", "TS", "STREAM_DATA", "PACKET")
DIR_NO_SERVICE, DIR_NO_COMPONENT, DIR_NO_PKTCOMP, DIR_NO_SUBCH = -2, -3, -4, -5
DIR_STATS = ("frames", "frames_without_fic", "frames_skipped", "fibs", "fibs_crc_failed", "figs", "figs_truncated", "figs_ignored", "facts", "facts_changed",
             "overflow_dropped")
DIR_STAGES = ("fibs", "merge")


class DirUnresolved(DabhipError):
    """Dir.resolve met a missing link; .code is DIR_NO_SERVICE, DIR_NO_COMPONENT, DIR_NO_PKTCOMP or DIR_NO_SUBCH."""

    def __init__(self, code, text):
        super().__init__(text)
        self.code = code


class Dir(_Handle):
    """The ensemble directory out of ETI frames on the GPU (dabhip_dir_*): per stream, the ensemble record, the sub-channels, the services with
    their components and labels, the packet components, from the FIC bytes of the frames pushed.  plan() names what DabPlus, Packet and Ts ask for."""
    _destroy = "dabhip_dir_destroy"

    def __init__(self, nstreams=1, device=0):
        self.nstreams = int(nstreams)
        self._h = lib().dabhip_dir_create(device, self.nstreams)
        _need(self._h, "dir_create")

    def push(self, frames, counts=None):
        """frames as Ts.push takes them.  Returns the FIBs of this push whose CRC held."""
        src, cnt, on_dev, keep = _eti_frames_arg("dir_push", self.nstreams, frames, counts)
        if keep is not None:
            self._keep = keep
        n = lib().dabhip_dir_push(self._h, src, cnt, on_dev)
        _need(n >= 0, "dir_push")
        return n

    def ensemble(self, stream=0):
        """The ensemble record: a DIR_ENSEMBLE scalar."""
        out = np.zeros(1, dtype=DIR_ENSEMBLE)
        _need(lib().dabhip_dir_ensemble(self._h, stream, out.ctypes.data) == 0, "dir_ensemble")
        return out[0]

    def _table(self, fn, what, dtype, stream):
        out = np.zeros(64, dtype=dtype)
        n = fn(self._h, stream, out.ctypes.data, 64)
        _need(0 <= n <= 64, what)
        return out[:n]

    def subchannels(self, stream=0):
        """Sub-channels with any part, in SubChId order: a DIR_SUBCH array."""
        return self._table(lib().dabhip_dir_subchannels, "dir_subchannels", DIR_SUBCH, stream)

    def services(self, stream=0):
        """Services in order of first appearance: a DIR_SERVICE array."""
        return self._table(lib().dabhip_dir_services, "dir_services", DIR_SERVICE, stream)

    def packet_components(self, stream=0):
        """Packet components in order of first appearance: a DIR_PKTCOMP array."""
        return self._table(lib().dabhip_dir_packet_components, "dir_packet_components", DIR_PKTCOMP, stream)

    def complete(self, stream=0):
        r = lib().dabhip_dir_complete(self._h, stream)
        _need(r >= 0, "dir_complete")
        return bool(r)

    def resolve(self, stream, pd, sid, component=0):
        """{kind (a DIR_KINDS name), subch, address, dg, dscty, fec, scid, primary}; DirUnresolved when a link is missing."""
        out = np.zeros(1, dtype=DIR_TARGET)
        r = lib().dabhip_dir_resolve(self._h, stream, int(pd), int(sid), int(component), out.ctypes.data)
        if r in (DIR_NO_SERVICE, DIR_NO_COMPONENT, DIR_NO_PKTCOMP, DIR_NO_SUBCH):
            raise DirUnresolved(r, last_error())
        _need(r == 0, "dir_resolve")
        t = {n: int(out[0][n]) for n in DIR_TARGET.names}
        t["kind"] = DIR_KINDS[t["kind"]]
        t["fec"] = bool(t["fec"])
        return t

    def reset(self, stream=0):
        _need(lib().dabhip_dir_reset(self._h, stream) == 0, "dir_reset")

    def stats(self, stream=0):
        """Counters since creation, in DIR_STATS order (int64 array of 11)."""
        c = np.zeros(11, dtype=np.int64)
        _need(lib().dabhip_dir_stats(self._h, stream, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "dir_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push per stage: DIR_STAGES in ms."""
        return _stage_ms(lib().dabhip_dir_stage_ms, self._h, len(DIR_STAGES))

    def plan(self, stream=0):
        """One dict per component that resolves, services in table order: sid, pd, component, label (16 bytes), kind, subch, fec, address -- what
        DabPlus(nstreams, [subch]), Packet(nstreams, [subch], fec=[fec]) and Ts(nstreams, [subch]) are built from."""
        out = []
        for s in self.services(stream):
            for c in range(int(s["ncomp"])):
                try:
                    t = self.resolve(stream, int(s["pd"]), int(s["sid"]), c)
                except DirUnresolved:
                    continue
                out.append({"sid": int(s["sid"]), "pd": int(s["pd"]), "component": c, "label": bytes(s["label"]), "kind": t["kind"], "subch": t["subch"],
                            "fec": t["fec"], "address": t["address"]})
        return out


# ---- EDI out of ETI (dabhip.h: dabhip_edi_*) --------------------------------------------------------------------------------
EDI_REC = np.dtype([("offset", "<i8"), ("frame", "<i8"), ("length", "<i4"), ("findex", "<i4"), ("fcount", "<i4"), ("seq", "<u2"), ("pad", "<u2")])
EDI_SIZES = np.dtype([(n, "<i4") for n in ("c", "k", "z", "B", "f", "s")])
assert (EDI_REC.itemsize, EDI_SIZES.itemsize) == (32, 24)
EDI_AF, EDI_PFT, EDI_PFT_FEC = 0, 1, 2
EDI_STATS = ("frames", "frames_skipped", "frames_without_fic", "packets", "bytes_out", "chunks_encoded")
EDI_STAGES = ("plan", "scan", "assemble", "rs", "fragment")


def edi_plan(l, mode=EDI_PFT_FEC, recover=0, max_frag=1400):
    """The sizes of one AF packet of l bytes by the function the kernels use (host only): {c, k, z, B, f, s}.  DabhipError on a refused argument."""
    out = np.zeros(1, dtype=EDI_SIZES)
    _need(lib().dabhip_edi_plan(int(l), int(mode), int(recover), int(max_frag), out.ctypes.data) == 0, "edi_plan")
    return {n: int(out[0][n]) for n in EDI_SIZES.names}


class Edi(_Handle):
    """EDI packets out of ETI frames on the GPU (dabhip_edi_*): every frame as TAG items in an AF packet (mode EDI_AF), cut into PFT fragments
    (EDI_PFT), or protected by RS(255,207) and interleaved over the fragments (EDI_PFT_FEC), for nstreams streams.  FCTH and SEQ carry from push
    to push."""
    _destroy = "dabhip_edi_destroy"

    def __init__(self, nstreams=1, mode=EDI_AF, recover=0, max_frag=1400, seq0=0, device=0):
        self.nstreams, self.mode = int(nstreams), int(mode)
        self._h = lib().dabhip_edi_create(device, self.nstreams, self.mode, int(recover), int(max_frag), int(seq0))
        _need(self._h, "edi_create")

    def push(self, frames, counts=None):
        """frames as Ts.push takes them.  Returns the packets of this push."""
        src, cnt, on_dev, keep = _eti_frames_arg("edi_push", self.nstreams, frames, counts)
        if keep is not None:
            self._keep = keep
        n = lib().dabhip_edi_push(self._h, src, cnt, on_dev)
        _need(n >= 0, "edi_push")
        return n

    def records(self, stream=0):
        """Records of the last push's packets of a stream: an EDI_REC array."""
        return _fetch(lib().dabhip_edi_records, "edi_records", EDI_REC, self._h, stream)

    def data(self, stream=0):
        """Their bytes, packet after packet: a uint8 array."""
        return _fetch(lib().dabhip_edi_data, "edi_data", np.uint8, self._h, stream)

    def reset(self, stream=0):
        _need(lib().dabhip_edi_reset(self._h, stream) == 0, "edi_reset")

    def stats(self, stream=0):
        """Counters since creation, in EDI_STATS order (int64 array of 6)."""
        c = np.zeros(6, dtype=np.int64)
        _need(lib().dabhip_edi_stats(self._h, stream, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "edi_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push per stage: EDI_STAGES in ms."""
        return _stage_ms(lib().dabhip_edi_stage_ms, self._h, len(EDI_STAGES))


# ---- EDI in (dabhip.h: dabhip_edirx_*) ----------------------------------------------------------------------------------------
EDIRX_REC = np.dtype([("frame", "<i8"), ("received", "<i4"), ("expected", "<i4"), ("words_filled", "<i4"), ("erasures_filled", "<i4"), ("seq", "<u2"),
                      ("fcth", "u1"), ("fct", "u1"), ("pad", "<u4")])
assert EDIRX_REC.itemsize == 32
EDIRX_STATS = ("packets", "bad_packets", "late", "duplicates", "mismatched", "missing", "groups_incomplete", "groups_rs_failed", "groups_crc_failed",
               "groups_refused", "words_filled", "erasures_filled", "items_ignored", "with_atst", "frames")
EDIRX_STAGES = ("parse", "window", "gather", "rs", "frame", "emit", "carry")


class EdiRx(_Handle):
    """ETI frames out of EDI packets on the GPU (dabhip_edirx_*): AF packets as they are, PFT fragments reassembled within a window of `depth`
    sequence numbers, lost fragments recovered by RS(255,207) erasure decoding, for nstreams streams.  The window and the held fragments
    carry from push to push."""
    _destroy = "dabhip_edirx_destroy"

    def __init__(self, nstreams=1, depth=4, device=0):
        self.nstreams = int(nstreams)
        self._h = lib().dabhip_edirx_create(device, self.nstreams, int(depth))
        _need(self._h, "edirx_create")

    def push(self, packets, counts=None):
        """packets: the datagrams (bytes or uint8 arrays) of all streams, stream after stream, counts[s] of stream s (one stream: all of them);
        or a tuple (device pointer, lengths, counts) of their bytes concatenated in device memory.  Returns the ETI frames of this push."""
        if isinstance(packets, tuple):
            ptr, lengths, counts = packets
            src, on_dev = C.c_void_p(ptr), 1
        else:
            packets = [np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8).reshape(-1) for x in packets]
            lengths = [x.size for x in packets]
            if counts is None:
                counts = _one_stream_counts("edirx_push", self.nstreams, len(packets))
            _need(sum(int(c) for c in counts) == len(packets), "edirx_push: counts and packets disagree")
            arr = np.ascontiguousarray(np.concatenate(packets)) if packets else np.zeros(0, np.uint8)
            self._keep = arr
            src, on_dev = C.c_void_p(arr.ctypes.data), 0
        _need(len(counts) == self.nstreams, "edirx_push: one count per stream")
        _need(sum(int(c) for c in counts) == len(lengths), "edirx_push: counts and lengths disagree")
        cnt = (C.c_int64 * self.nstreams)(*[int(c) for c in counts])
        lens = np.ascontiguousarray(lengths, dtype=np.int32)
        n = lib().dabhip_edirx_push(self._h, src, lens.ctypes.data_as(C.POINTER(C.c_int32)), cnt, on_dev)
        _need(n >= 0, "edirx_push")
        return n

    def flush(self, stream=-1):
        """Finalises the open groups of a stream (-1: of all).  Returns the frames this gave."""
        n = lib().dabhip_edirx_flush(self._h, int(stream))
        _need(n >= 0, "edirx_flush")
        return n

    def records(self, stream=0):
        """Records of the last push's or flush's frames of a stream: an EDIRX_REC array."""
        n = lib().dabhip_edirx_records(self._h, stream, None, 0)
        _need(n >= 0, "edirx_records")
        out = np.zeros(n, dtype=EDIRX_REC)
        _need(lib().dabhip_edirx_records(self._h, stream, out.ctypes.data, n) == n, "edirx_records")
        return out

    def frames(self, stream=0):
        """Their bytes: a uint8 array (n, 6144)."""
        n = lib().dabhip_edirx_frames(self._h, stream, None, 0)
        _need(n >= 0, "edirx_frames")
        out = np.zeros((n, ETI_BYTES), dtype=np.uint8)
        _need(lib().dabhip_edirx_frames(self._h, stream, _p(out), out.size) == n, "edirx_frames")
        return out

    def reset(self, stream=0):
        _need(lib().dabhip_edirx_reset(self._h, stream) == 0, "edirx_reset")

    def stats(self, stream=0):
        """Counters since creation, in EDIRX_STATS order (int64 array of 15)."""
        c = np.zeros(len(EDIRX_STATS), dtype=np.int64)
        _need(lib().dabhip_edirx_stats(self._h, stream, c.ctypes.data_as(C.POINTER(C.c_int64)), c.size) == c.size, "edirx_stats")
        return c

    def stage_ms(self):
        """GPU time of the last push or flush per stage: EDIRX_STAGES in ms."""
        return _stage_ms(lib().dabhip_edirx_stage_ms, self._h, len(EDIRX_STAGES))


class PacketGroups(_Handle):
    """MSC data groups out of the packets of one (stream, sub-channel) on the host (dabhip_packet_groups_*).  State carries from push to push."""
    _destroy = "dabhip_packet_groups_destroy"

    def __init__(self):
        self._h = lib().dabhip_packet_groups_create()
        _need(self._h, "packet_groups_create")

    def push(self, records, data):
        """The records and useful bytes of a push (Packet.records / .data) -> [(PACKET_GROUP record, bytes)] of the groups they complete."""
        recs = np.ascontiguousarray(records, dtype=PACKET_REC)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = lib().dabhip_packet_groups_push(self._h, recs.ctypes.data, recs.size, _p(data), data.size)
        _need(n >= 0, "packet_groups_push")
        out = []
        for i in range(n):
            rec = np.zeros(1, dtype=PACKET_GROUP)
            size = lib().dabhip_packet_groups_get(self._h, i, rec.ctypes.data, None, 0)
            _need(size >= 0, "packet_groups_get")
            buf = np.zeros(size, dtype=np.uint8)
            _need(lib().dabhip_packet_groups_get(self._h, i, None, _p(buf), size) == size, "packet_groups_get")
            out.append((rec[0], buf))
        return out

    def stats(self):
        """Counters since creation, in PACKET_GROUP_STATS order (int64 array of 4)."""
        c = np.zeros(4, dtype=np.int64)
        _need(lib().dabhip_packet_groups_stats(self._h, c.ctypes.data_as(C.POINTER(C.c_int64))) == 0, "packet_groups_stats")
        return c


# ---- ingest stage: other sample formats and rates -> cu8 at 2.048 Msps (dabhip.h: dabhip_ingest_*) -----------------
INGEST_FORMATS = {"cu8": 0, "cs8": 1, "cs16": 2, "cf32": 3}
INGEST_DTYPES = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.dtype("<i2"), "cf32": np.dtype("<f4")}
INGEST_GAIN_WINDOW = 65536


def _ingest_format(fmt):
    if isinstance(fmt, str):
        if fmt not in INGEST_FORMATS:
            raise DabhipError("ingest: unknown format %r (cu8, cs8, cs16, cf32)" % fmt)
        return INGEST_FORMATS[fmt]
    return int(fmt)


def _ingest_taps(name, fmt, rate):
    fn = getattr(lib(), "dabhip_" + name)
    L, M, T = C.c_int(0), C.c_int(0), C.c_int(0)
    n = fn(_ingest_format(fmt), int(rate), None, 0, C.byref(L), C.byref(M), C.byref(T))
    _need(n >= 0, name)
    taps = np.zeros(n, dtype=np.int16)
    if n:
        _need(fn(_ingest_format(fmt), int(rate), taps.ctypes.data_as(C.POINTER(C.c_int16)), n, None, None, None) == n, name)
    return taps.reshape(L.value, T.value), L.value, M.value, T.value


def _ingest_plan(name, rate, pushes, auto_gain):
    n = len(pushes)
    src = (C.c_int64 * max(n, 1))(*[int(v) for v in pushes])
    nout, keep = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
    _need(getattr(lib(), "dabhip_" + name)(int(rate), 1 if auto_gain else 0, src, n, nout, keep) == 0, name)
    return list(nout)[:n], list(keep)[:n]


def ingest_taps(fmt, rate):
    """(taps [L][T] int16 in Q14, L, M, T) of a sample rate (dabhip_ingest_taps; no GPU needed).  L/M = 1/1: an empty table, T = 0."""
    return _ingest_taps("ingest_taps", fmt, rate)


def ingest_plan(rate, pushes, auto_gain=False):
    """The bookkeeping of one stream over pushes of `pushes` samples: (output samples completed per push, input samples carried behind each)."""
    return _ingest_plan("ingest_plan", rate, pushes, auto_gain)


def ingest_tune_taps(fmt, rate):
    """ingest_taps of the tuned mode: twice the taps, cut-off 856 kHz (dabhip_ingest_tune_taps)."""
    return _ingest_taps("ingest_tune_taps", fmt, rate)


def ingest_tune_plan(rate, pushes, auto_gain=False):
    """ingest_plan of the tuned mode: the gain window closes on outputs (dabhip_ingest_tune_plan)."""
    return _ingest_plan("ingest_tune_plan", rate, pushes, auto_gain)


def ingest_tune_nco():
    """The tuned mode's mixer table: int16 [4096][2], (cos, sin) in Q14 (dabhip_ingest_tune_nco)."""
    cs = np.zeros((4096, 2), dtype=np.int16)
    _need(lib().dabhip_ingest_tune_nco(cs.ctypes.data_as(C.POINTER(C.c_int16)), 4096) == 4096, "ingest_tune_nco")
    return cs


def ingest_tune_step(rate, offset_hz):
    """The mixer's phase step per input sample, in 2^-32 turns, of a channel offset_hz from the capture's centre (dabhip_ingest_tune_step)."""
    step = C.c_uint32(0)
    _need(lib().dabhip_ingest_tune_step(int(rate), int(offset_hz), C.byref(step)) == 0, "ingest_tune_step")
    return step.value


def ingest_auto_gain(energy):
    """The automatic gain of an energy sum(I^2 + Q^2) over the first 65536 samples in the 16-bit domain (dabhip.h, step 4)."""
    return lib().dabhip_ingest_auto_gain(int(energy))


class Ingest(_Handle):
    """nstreams streams of fmt ("cu8", "cs8", "cs16", "cf32") IQ at `rate` samples/s -> cu8 at 2.048 Msps in device memory (dabhip_ingest_*).
    gain: the requantisation gain (256 = 16-bit full scale to 8-bit full scale), 0 = automatic.  State carries from push to push.
    offsets: the tuned mode (dabhip_ingest_create_tuned) -- every input stream gives len(offsets) output streams, channel c the DAB block centred
    offsets[c] Hz from the capture's centre; output stream `stream * nchannels + channel` is what output_ptrs, read and gain index."""
    _destroy = "dabhip_ingest_destroy"

    def __init__(self, device, nstreams, fmt, rate, gain=0, offsets=None):
        self.nstreams, self.fmt = int(nstreams), _ingest_format(fmt)
        if offsets is None:
            self.nchannels = 1
            self._h = lib().dabhip_ingest_create(int(device), self.nstreams, self.fmt, int(rate), int(gain))
            _need(self._h, "ingest_create")
        else:
            self.nchannels = len(offsets)
            off = (C.c_int64 * max(self.nchannels, 1))(*[int(f) for f in offsets])
            self._h = lib().dabhip_ingest_create_tuned(int(device), self.nstreams, self.fmt, int(rate), int(gain), off, self.nchannels)
            _need(self._h, "ingest_create_tuned")
        self.nouts = self.nstreams * self.nchannels

    def push(self, arrays):
        """One array per stream (any dtype: its bytes are the samples, possibly none) -> total output bytes of this push."""
        self._keep = arrs = _sample_bytes("ingest_push", self.nstreams, arrays)
        return self.push_ptrs([a.ctypes.data for a in arrs], [a.size for a in arrs], on_device=False)

    def push_ptrs(self, ptrs, sizes, on_device=False):
        """push() over raw addresses: host memory, or device memory aligned to a sample."""
        return _push_samples(lib().dabhip_ingest_push, "ingest_push", self._h, self.nstreams, ptrs, sizes, on_device)

    def output_ptrs(self):
        """(device addresses, byte counts) of this push's cu8, per output stream: what Engine.decode_device and Stream.feed_ptrs(on_device=True) take.
        Valid until the next push."""
        ptrs, sizes = [], []
        for b in range(self.nouts):
            p, n = C.c_void_p(0), C.c_size_t(0)
            _need(lib().dabhip_ingest_output(self._h, b, C.byref(p), C.byref(n)) == 0, "ingest_output")
            ptrs.append(p.value or 0)
            sizes.append(n.value)
        return ptrs, sizes

    def read(self, stream):
        """This push's cu8 of one stream as a numpy array."""
        p, n = C.c_void_p(0), C.c_size_t(0)
        _need(lib().dabhip_ingest_output(self._h, stream, C.byref(p), C.byref(n)) == 0, "ingest_output")
        out = np.zeros(n.value, dtype=np.uint8)
        _need(lib().dabhip_ingest_read(self._h, stream, _p(out), out.size) == out.size, "ingest_read")
        return out

    def gain(self, stream):
        """The stream's gain; 0 while its automatic-gain window is open."""
        return lib().dabhip_ingest_gain(self._h, stream)

    def skip(self, n):
        """Test knob (explicit gain only): as if n zero samples had been pushed to every stream and their outputs discarded."""
        _need(lib().dabhip_ingest_skip(self._h, int(n)) == 0, "ingest_skip")

    def stage_ms(self):
        """GPU time of the last push per stage: {"upload", "energy", "resample", "keep"} in ms."""
        return _stage_ms(lib().dabhip_ingest_stage_ms, self._h, 4)


# ---- block scan: which DAB blocks lie in a wideband capture (dabhip.h: dabhip_scan_*) ------------------------------
SCAN_BINS = 4096
SCAN_DEFAULT_SEGMENTS = 64


class ScanBlockRecord(C.Structure):
    """dabhip_scan_block."""
    _fields_ = [("offset_hz", C.c_int64), ("raw_center_hz", C.c_int64), ("width_hz", C.c_int64), ("in_", C.c_uint64), ("lo", C.c_uint64), ("hi", C.c_uint64),
                ("nin", C.c_int32), ("ng", C.c_int32), ("name", C.c_char * 8)]


def _scan_records(recs, n):
    """The first n records as dicts: offset_hz, raw_center_hz, width_hz, name ("" = off the raster), in, lo, hi (sums), nin, ng (their bin counts)."""
    return [{"offset_hz": r.offset_hz, "raw_center_hz": r.raw_center_hz, "width_hz": r.width_hz, "name": r.name.decode(), "in": r.in_, "lo": r.lo, "hi": r.hi,
             "nin": r.nin, "ng": r.ng} for r in recs[:n]]


def scan_detect(P, rate, center=0):
    """The blocks in a power spectrum of 4096 bins in transform order (dabhip_scan_detect; no GPU needed): a list of records in ascending offset.
    center: the capture's centre frequency in Hz, 0 = not known (no snapping to the Band III raster)."""
    P = np.ascontiguousarray(P, dtype=np.uint64).reshape(-1)
    _need(P.size == SCAN_BINS, "scan_detect: a spectrum of 4096 bins is wanted")
    recs = (ScanBlockRecord * 16)()
    n = lib().dabhip_scan_detect(P.ctypes.data_as(C.POINTER(C.c_uint64)), int(rate), int(center), C.cast(recs, C.c_void_p), 16)
    _need(n >= 0, "scan_detect")
    return _scan_records(recs, n)


def scan_plan(nsegments, pushes):
    """The bookkeeping of one stream of a Scan over pushes of `pushes` samples: (segments completed per push, samples carried behind each)."""
    n = len(pushes)
    src = (C.c_int64 * max(n, 1))(*[int(v) for v in pushes])
    nseg, keep = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
    _need(lib().dabhip_scan_plan(int(nsegments), src, n, nseg, keep) == 0, "scan_plan")
    return list(nseg)[:n], list(keep)[:n]


class Scan(_Handle):
    """The power spectrum of the first nsegments segments of 4096 samples of nstreams streams of fmt IQ at `rate` samples/s, and the DAB blocks in
    it (dabhip_scan_*).  State carries from push to push; samples past the window are ignored."""
    _destroy = "dabhip_scan_destroy"

    def __init__(self, device, nstreams, fmt, rate, nsegments=SCAN_DEFAULT_SEGMENTS):
        self.nstreams, self.fmt, self.rate = int(nstreams), _ingest_format(fmt), int(rate)
        self._h = lib().dabhip_scan_create(int(device), self.nstreams, self.fmt, self.rate, int(nsegments))
        _need(self._h, "scan_create")

    def push(self, arrays):
        """One array per stream (any dtype: its bytes are the samples, possibly none) -> segments accumulated by this push over all streams."""
        self._keep = arrs = _sample_bytes("scan_push", self.nstreams, arrays)
        return self.push_ptrs([a.ctypes.data for a in arrs], [a.size for a in arrs], on_device=False)

    def push_ptrs(self, ptrs, sizes, on_device=False):
        """push() over raw addresses: host memory, or device memory aligned to a sample."""
        return _push_samples(lib().dabhip_scan_push, "scan_push", self._h, self.nstreams, ptrs, sizes, on_device)

    def spectrum(self, stream):
        """(P: uint64 [4096] in transform order, segments accumulated) of one stream."""
        P = np.zeros(SCAN_BINS, dtype=np.uint64)
        done = C.c_int(0)
        _need(lib().dabhip_scan_spectrum(self._h, int(stream), P.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(done)) == 0, "scan_spectrum")
        return P, done.value

    def blocks(self, stream, center=0):
        """The blocks of one stream as scan_detect gives them."""
        recs = (ScanBlockRecord * 16)()
        n = lib().dabhip_scan_blocks(self._h, int(stream), int(center), C.cast(recs, C.c_void_p), 16)
        _need(n >= 0, "scan_blocks")
        return _scan_records(recs, n)

    def stage_ms(self):
        """GPU time of the last push per stage: {"upload", "transform", "keep"} in ms."""
        return _stage_ms(lib().dabhip_scan_stage_ms, self._h, 3)


# ---- TII: which transmitters an ensemble comes from (dabhip.h: "TII") ---------------------------------------------
TII_SUMS = 192
TII_SHADOW = 1


class TiiRecord(C.Structure):
    """dabhip_tii_id."""
    _fields_ = [("main_id", C.c_int32), ("sub_id", C.c_int32), ("flags", C.c_uint32), ("pad", C.c_int32), ("strong", C.c_uint64), ("weak", C.c_uint64)]


def _tii_records(recs, n):
    """The first n records as dicts: main, sub, shadow (the DABHIP_TII_SHADOW flag), strong, weak (s and n of the rule)."""
    return [{"main": r.main_id, "sub": r.sub_id, "shadow": bool(r.flags & TII_SHADOW), "strong": r.strong, "weak": r.weak} for r in recs[:n]]


def tii_detect(T):
    """The transmitters in 192 folded sums T[8 c + b] (dabhip_tii_detect; no GPU needed): a list of records in ascending sub identifier."""
    T = np.ascontiguousarray(T, dtype=np.uint64).reshape(-1)
    _need(T.size == TII_SUMS, "tii_detect: 192 sums are wanted")
    recs = (TiiRecord * 24)()
    n = lib().dabhip_tii_detect(T.ctypes.data_as(C.POINTER(C.c_uint64)), C.cast(recs, C.c_void_p), 24)
    _need(n >= 0, "tii_detect")
    return _tii_records(recs, n)


def tii_carriers(main_id, sub_id):
    """The 32 carriers of transmitter (main_id, sub_id) (dabhip_tii_carriers; no GPU needed)."""
    k = np.zeros(32, dtype=np.int16)
    _need(lib().dabhip_tii_carriers(int(main_id), int(sub_id), k.ctypes.data_as(C.POINTER(C.c_int16)), 32) == 32, "tii_carriers")
    return k


def _tii_sums(fn, h, stream):
    T = np.zeros(TII_SUMS, dtype=np.uint64)
    frames = C.c_int(0)
    _need(fn(h, int(stream), T.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(frames)) == 0, "tii_sums")
    return T, frames.value


def _tii_ids(fn, h, stream):
    recs = (TiiRecord * 24)()
    n = fn(h, int(stream), C.cast(recs, C.c_void_p), 24)
    _need(n >= 0, "tii")
    return _tii_records(recs, n)


class Engine(_Handle):
    def __init__(self, device=0, host_threads=0, _borrowed=None):
        self._owned = _borrowed is None
        self._h = _borrowed or lib().dabhip_engine_create_ex(device, host_threads)
        _need(self._h, "engine_create")
        self.nstreams = 0

    def set_afc(self, enable):
        """Software AFC (NCO per stream steered by the reference's tuner rule); off = parity mode."""
        _need(lib().dabhip_engine_set_afc(self._h, 1 if enable else 0) == 0, "set_afc")

    def set_soft(self, enable):
        """Soft-decision decoding (4-bit soft values into the Viterbi metrics); off = parity mode."""
        _need(lib().dabhip_engine_set_soft(self._h, 1 if enable else 0) == 0, "set_soft")

    def set_decoder_forms(self, msc=None, fic=None):
        """Force the Viterbi form of every MSC / FIC launch (names or FORM_* numbers; None = the default rule, engine.hpp)."""
        _need(lib().dabhip_engine_set_decoder_forms(self._h, _form(msc), _form(fic)) == 0, "set_decoder_forms")

    def set_soft_lanes(self, enable):
        """Let soft decisions run the four-lane and table-free two-lane decoder forms (dabhip.h; default off: a soft engine runs the lane
        form whatever is forced).  Any time; changes which kernel a later launch takes, never the bytes."""
        _need(lib().dabhip_engine_set_soft_lanes(self._h, 1 if enable else 0) == 0, "set_soft_lanes")

    def decoder_forms(self, masks=False):
        """The forms that ran since the last decode / stage_fic_decode began: ({MSC form names}, {FIC form names}), or the two bit masks."""
        m, f = _decoder_forms(lib().dabhip_engine_decoder_forms, self._h)
        return (m, f) if masks else (_form_names(m), _form_names(f))

    def set_subchannels(self, ids):
        """Decode and carry only these SubChIds (None / empty = all, the reference's frames)."""
        ids = list(ids or [])
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        _need(lib().dabhip_engine_set_subchannels(self._h, arr, len(ids)) == 0, "set_subchannels")

    def set_fused(self, enable):
        """True (default): one kernel for OFDM transform + demap (spectra never written); False: K2 + K2b.  Identical output."""
        _need(lib().dabhip_engine_set_fused(self._h, 1 if enable else 0) == 0, "set_fused")

    def set_demod_all(self, on):
        """Lock-in skip off switch: True = the MSC symbols of every TF are demodulated, also of those that cannot be locked (dabhip.h).  Identical ETI."""
        _need(lib().dabhip_engine_set_demod_all(self._h, 1 if on else 0) == 0, "set_demod_all")

    def msc_deferred(self):
        """TFs of the last decode whose MSC symbols were deferred by the lock-in skip (demapped_tf completes them on demand)."""
        n = lib().dabhip_engine_msc_deferred(self._h)
        _need(n >= 0, "msc_deferred")
        return n

    def set_sync_speculation(self, mode):
        """K1's chain: 0 = call after call, 1 = with the look-ahead pass, -1 (default) = the pass for small batches.  Identical results."""
        _need(lib().dabhip_engine_set_sync_speculation(self._h, int(mode)) == 0, "set_sync_speculation")

    def set_parity_guard(self, level=True):
        """Decisions inside the fp32 error band are re-decided in fp64 -> bits of exact arithmetic.  level: False / 0 = off, 1 = the measured
        band, 2 = the proven band, True = the library's default level (dabhip.h: DABHIP_GUARD_*)."""
        _need(lib().dabhip_engine_set_parity_guard(self._h, _guard_level(level)) == 0, "set_parity_guard")

    def parity_guard_level(self):
        return lib().dabhip_engine_parity_guard_level(self._h)

    def guard_stats(self):
        """(decisions re-decided by the parity guard, hard decisions taken) of the last decode."""
        a, b = C.c_int64(0), C.c_int64(0)
        _need(lib().dabhip_engine_guard_stats(self._h, C.byref(a), C.byref(b)) == 0, "guard_stats")
        return a.value, b.value

    def guard_overflows(self):
        """Launches of the last decode whose guard list overflowed (their frames were decided again in full, in fp64)."""
        return lib().dabhip_engine_guard_overflows(self._h)

    def set_guard_list_cap(self, cap):
        """Test knob: capacity of the guard's list per launch (0 = automatic)."""
        _need(lib().dabhip_engine_set_guard_list_cap(self._h, cap) == 0, "set_guard_list_cap")

    def set_launch_limits(self, **limits):
        """Test knob: the sizes past which a decode is split into several launches (LAUNCH_LIMITS; a limit left out or 0 = its default).  The output
        does not depend on them.  A value no launch could be made with is refused (DabhipError) and the limits stay as they were."""
        _set_launch_limits(lib().dabhip_engine_set_launch_limits, self._h, limits)

    def launch_report(self):
        """{loop: launches it made} of the last decode / stage entry (LAUNCH_REPORT), and how the scan's results came back (fetch_form: FETCH_*)."""
        return _launch_report(lib().dabhip_engine_launch_report, self._h)

    def msc_plan(self):
        """(trellis steps of every wave-group of the last decode's MSC batch in launch order, tiles of 64 records its regroup covers): dabhip_engine_msc_plan"""
        tiles = C.c_int64(0)
        n = lib().dabhip_engine_msc_plan(self._h, None, 0, C.byref(tiles))
        _need(n >= 0, "msc_plan")
        steps = np.zeros(max(n, 1), dtype=np.int32)
        _need(lib().dabhip_engine_msc_plan(self._h, steps.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(tiles)) == n, "msc_plan")
        return steps[:n], tiles.value

    def decision_audit(self, frames=None, device_ptr=None, nframes=None, guard=False, fused=False):
        """fp32 OFDM stage vs fp64 on contiguous cu8 frames -> dict (see dabhip_stage_decision_audit); fused: the default decode's one-kernel stage
        (dabhip_stage_decision_audit_fused) instead of K2 + K2b."""
        if device_ptr is None:
            frames = np.ascontiguousarray(frames, dtype=np.uint8)
            nframes = frames.size // TF_BYTES
            src, on_dev = frames.ctypes.data, 0
        else:
            src, on_dev = device_ptr, 1
        keys = ("decisions", "disagree", "disagree_outside_guard", "flagged_by_rule", "max_bin_err", "max_dec_err", "max_prod_err", "listed")
        if fused:
            out = (C.c_double * 10)()
            _need(lib().dabhip_stage_decision_audit_fused(self._h, src, nframes, on_dev, 1 if guard else 0, out) == nframes, "stage_decision_audit_fused")
            d = dict(zip(keys, list(out)[:8]))
            d["shipping_kernel_same_bits"], d["shipping_kernel_same_list_count"] = out[8], out[9]
            return d
        out = (C.c_double * 8)()
        _need(lib().dabhip_stage_decision_audit(self._h, src, nframes, on_dev, 1 if guard else 0, out) == nframes, "stage_decision_audit")
        return dict(zip(keys, list(out)))

    def decode(self, streams):
        """streams: list of numpy uint8 arrays (host) -> total ETI frames."""
        arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        n = lib().dabhip_engine_decode(self._h, ptrs, sizes, len(arrs), 0)
        _need(n >= 0, "engine_decode")
        self.nstreams = len(arrs)
        return n

    def decode_host_ptrs(self, ptrs, sizes):
        """ptrs: HOST addresses (ints; page-locked memory from HostBuffer uploads at the PCIe rate), sizes: byte counts."""
        p = (C.c_void_p * len(ptrs))(*ptrs)
        s = (C.c_size_t * len(sizes))(*sizes)
        n = lib().dabhip_engine_decode(self._h, p, s, len(ptrs), 0)
        _need(n >= 0, "engine_decode")
        self.nstreams = len(ptrs)
        return n

    def decode_device(self, ptrs, sizes):
        """ptrs: device addresses (ints, e.g. torch tensor.data_ptr()), sizes: byte counts."""
        return self.decode_marshalled(self.marshal(ptrs, sizes), on_device=True)

    @staticmethod
    def marshal(ptrs, sizes):
        """The C argument arrays of a decode, built once for callers that decode the same buffers again and again."""
        return (C.c_void_p * len(ptrs))(*ptrs), (C.c_size_t * len(sizes))(*sizes), len(ptrs)

    def decode_marshalled(self, args, on_device=True):
        p, s, n_streams = args
        n = lib().dabhip_engine_decode(self._h, p, s, n_streams, 1 if on_device else 0)
        _need(n >= 0, "engine_decode")
        self.nstreams = n_streams
        return n

    def eti(self, stream):
        n = lib().dabhip_engine_eti_count(self._h, stream)
        _need(n >= 0, "eti_count")
        out = np.zeros((n, ETI_BYTES), dtype=np.uint8)
        if n:
            _need(lib().dabhip_engine_eti_read(self._h, stream, _p(out), n) == n, "eti_read")
        return out

    def eti_count(self, stream):
        return lib().dabhip_engine_eti_count(self._h, stream)

    def stream_status(self, stream):
        """dabhip_engine_stream_status: 0 = fine, else STREAM_* fault bits (the stream emitted no frames while its multiplex was un-assemblable)."""
        return int(lib().dabhip_engine_stream_status(self._h, stream))

    def log(self, stream):
        """The reference's operator messages for one stream of the last decode, cleared by the call (dabhip_engine_stream_log): 'Locked' (dab.c:51),
        'Lock lost, resetting ringbuffer' (dab.c:57), the one-time ensemble dump (dab.c:78-82, misc.c:316-328)."""
        buf = C.create_string_buffer(1 << 16)
        _need(lib().dabhip_engine_stream_log(self._h, stream, buf, len(buf)) >= 0, "engine_stream_log")
        return buf.value.decode("ascii")

    def eti_fetch(self, dst_ptr, cap_frames):
        """dabhip_engine_eti_fetch: all frames of the last decode (stream-major) on their way to (page-locked) host memory."""
        n = lib().dabhip_engine_eti_fetch(self._h, dst_ptr, cap_frames)
        _need(n >= 0, "eti_fetch")
        return n

    def eti_fetch_wait(self):
        _need(lib().dabhip_engine_eti_fetch_wait(self._h) == 0, "eti_fetch_wait")

    def demapped_tf(self, stream, tf):
        """(fic[9216], msc[221184]) int8: what the OFDM stage of the last decode left for that TF (0/1, or -7..7 with soft decisions)."""
        fic, msc = np.zeros(FIC_BITS, dtype=np.int8), np.zeros(MSC_BITS, dtype=np.int8)
        _need(lib().dabhip_engine_demapped_tf(self._h, stream, tf, fic.ctypes.data_as(C.POINTER(C.c_int8)), msc.ctypes.data_as(C.POINTER(C.c_int8))) == 0, "demapped_tf")
        return fic, msc

    def eti_device_ptr(self):
        n = C.c_int64(0)
        p = lib().dabhip_engine_eti_device_ptr(self._h, C.byref(n))
        return p, n.value

    def trace(self, stream, ncalls):
        ints = np.zeros((ncalls, 6), dtype=np.int32)
        ffs = np.zeros(ncalls, dtype=np.float64)
        n = lib().dabhip_engine_trace(self._h, stream, ints.ctypes.data_as(C.POINTER(C.c_int32)),
                                      ffs.ctypes.data_as(C.POINTER(C.c_double)), ncalls)
        _need(n >= 0, "engine_trace")
        return ints[:n], ffs[:n]

    def set_tii(self, enable):
        """Transmitter identification: every later decode also folds the null symbols of its frames onto the streams' sums; off by default."""
        _need(lib().dabhip_engine_set_tii(self._h, 1 if enable else 0) == 0, "set_tii")

    def tii_sums(self, stream):
        """(the 192 sums T[8 c + b] of one stream of the last decode, the frames that counted)"""
        return _tii_sums(lib().dabhip_engine_tii_sums, self._h, stream)

    def tii(self, stream):
        """The transmitters of one stream of the last decode as tii_detect gives them."""
        return _tii_ids(lib().dabhip_engine_tii, self._h, stream)

    def tii_ms(self):
        """GPU time of the TII kernel in the last decode, ms."""
        ms = C.c_float(0)
        _need(lib().dabhip_engine_tii_ms(self._h, C.byref(ms)) == 0, "tii_ms")
        return ms.value

    def stage_tii(self, frames, w0, step, device_ptr=None):
        """dabhip_stage_tii: contiguous frames (host array, or device_ptr) with a window start and a step each -> uint64 [nframes][192]."""
        w0 = np.ascontiguousarray(w0, dtype=np.int32)
        step = np.ascontiguousarray(step, dtype=np.uint32)
        n = w0.size
        _need(step.size == n, "stage_tii: one step per window")
        if device_ptr is None:
            frames = np.ascontiguousarray(frames, dtype=np.uint8)
            _need(frames.size == n * TF_BYTES, "stage_tii: whole frames, one per window")
            src, on_dev = frames.ctypes.data, 0
        else:
            src, on_dev = device_ptr, 1
        T = np.zeros((n, TII_SUMS), dtype=np.uint64)
        r = lib().dabhip_stage_tii(self._h, src, n, w0.ctypes.data_as(C.POINTER(C.c_int32)), step.ctypes.data_as(C.POINTER(C.c_uint32)), on_dev,
                                   T.ctypes.data_as(C.POINTER(C.c_uint64)))
        _need(r == n, "stage_tii")
        return T

    def trace_nco(self, stream, ncalls):
        """per call: the re-tuning in Hz the software AFC applied to that call's samples (dabhip_engine_trace_nco)"""
        out = np.zeros(ncalls, dtype=np.int32)
        n = lib().dabhip_engine_trace_nco(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_int32)), ncalls)
        _need(n >= 0, "trace_nco")
        return out[:n]

    def stage_ms(self):
        names = (C.c_char_p * 24)()
        ms = (C.c_float * 24)()
        n = lib().dabhip_engine_stage_ms(self._h, names, ms, 24)
        return {names[i].decode(): ms[i] for i in range(n)}

    def fft_stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_double(0)
        lib().dabhip_engine_fft_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def fft_roofline(self, reps=3):
        """K2 alone over the frames of the last decode -> (launches, TFs, total kernel ms)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_double(0)
        _need(lib().dabhip_engine_fft_roofline(self._h, reps, C.byref(a), C.byref(b), C.byref(c)) == 0, "fft_roofline")
        return a.value, b.value, c.value

    def stage_ofdm_fft(self, frames, reps=1, device_ptr=None, nframes=None, want_output=True):
        if device_ptr is None:
            frames = np.ascontiguousarray(frames, dtype=np.uint8)
            nframes = frames.size // TF_BYTES
            src, on_dev = frames.ctypes.data, 0
        else:
            src, on_dev = device_ptr, 1
        out = np.zeros((nframes, 76, 2048, 2), dtype=np.float32) if want_output else None
        ms = C.c_float(0)
        r = lib().dabhip_stage_ofdm_fft(self._h, src, nframes, out.ctypes.data_as(C.POINTER(C.c_float)) if want_output else None,
                                        on_dev, reps, C.byref(ms))
        _need(r == nframes, "stage_ofdm_fft")
        return out, ms.value

    def stage_demap(self, spectra):
        spectra = np.ascontiguousarray(spectra, dtype=np.float32)
        n = spectra.shape[0]
        fic = np.zeros((n, FIC_BITS), dtype=np.uint8)
        msc = np.zeros((n, MSC_BITS), dtype=np.uint8)
        _need(lib().dabhip_stage_demap(self._h, spectra.ctypes.data_as(C.POINTER(C.c_float)), n, _p(fic), _p(msc)) == n, "stage_demap")
        return fic, msc

    def stage_fic_decode(self, fic):
        fic = np.ascontiguousarray(fic, dtype=np.uint8).reshape(-1, FIC_BITS)
        n = fic.shape[0]
        fibs = np.zeros((n, 12, 32), dtype=np.uint8)
        ok = np.zeros((n, 12), dtype=np.uint8)
        _need(lib().dabhip_stage_fic_decode(self._h, _p(fic), n, _p(fibs), _p(ok)) == n, "stage_fic_decode")
        return fibs, ok

    def close(self):
        if self._h and self._owned:
            lib().dabhip_engine_destroy(self._h)
        self._h = None


class Multi(_Handle):
    """The batch engine over several devices of one node (dabhip_multi_*): streams dealt to the devices in contiguous slices
    (2048 on 8 = stream s on device s // 256), all slices decoding at once, no exchange between them.  A device may be listed
    several times (every entry is its own slice)."""
    _destroy = "dabhip_multi_destroy"

    def __init__(self, devices):
        devs = list(devices)
        self._h = lib().dabhip_multi_create((C.c_int * len(devs))(*devs), len(devs))
        _need(self._h, "multi_create")
        self.devices = devs
        self.nstreams = 0

    def _set(self, fn, enable):
        _need(fn(self._h, 1 if enable else 0) == 0, "multi_set")

    def set_afc(self, enable):
        self._set(lib().dabhip_multi_set_afc, enable)

    def set_soft(self, enable):
        self._set(lib().dabhip_multi_set_soft, enable)

    def set_soft_lanes(self, enable):
        """see Engine.set_soft_lanes"""
        self._set(lib().dabhip_multi_set_soft_lanes, enable)

    def set_parity_guard(self, level=True):
        _need(lib().dabhip_multi_set_parity_guard(self._h, _guard_level(level)) == 0, "multi_set_parity_guard")

    def set_fused(self, enable):
        self._set(lib().dabhip_multi_set_fused, enable)

    def set_subchannels(self, ids):
        ids = list(ids or [])
        _need(lib().dabhip_multi_set_subchannels(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids)) == 0, "multi_set_subchannels")

    def decode(self, streams):
        """streams: list of numpy uint8 arrays (host) -> total ETI frames."""
        arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in streams]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        n = lib().dabhip_multi_decode(self._h, ptrs, sizes, len(arrs), 0)
        _need(n >= 0, "multi_decode")
        self.nstreams = len(arrs)
        return n

    def decode_device(self, ptrs, sizes):
        """ptrs[b]: device address on the device of stream b's slice (slice_of)."""
        p = (C.c_void_p * len(ptrs))(*ptrs)
        s = (C.c_size_t * len(sizes))(*sizes)
        n = lib().dabhip_multi_decode(self._h, p, s, len(ptrs), 1)
        _need(n >= 0, "multi_decode")
        self.nstreams = len(ptrs)
        return n

    def plan(self, nstreams, stream):
        """(slice, device) that will decode `stream` of a batch of `nstreams` (dabhip_multi_plan: the dealing rule, before any decode)."""
        sl, dev = C.c_int(-1), C.c_int(-1)
        _need(lib().dabhip_multi_plan(self._h, nstreams, stream, C.byref(sl), C.byref(dev)) == 0, "multi_plan")
        return sl.value, dev.value

    def slice_cpus(self, slice_index):
        """(cpus, numa_node) the host threads of a slice are bound to ([] = unbound)."""
        buf, node = (C.c_int32 * 4096)(), C.c_int(-1)
        n = lib().dabhip_multi_slice_cpus(self._h, slice_index, buf, 4096, C.byref(node))
        _need(n >= 0, "multi_slice_cpus")
        return list(buf[:n]), node.value

    def slice_of(self, stream):
        """(slice, device) of a stream in a decode of the last decode's size."""
        dev = C.c_int(0)
        sl = lib().dabhip_multi_slice_of(self._h, stream, C.byref(dev))
        _need(sl >= 0, "multi_slice_of")
        return sl, dev.value

    def eti_count(self, stream):
        return lib().dabhip_multi_eti_count(self._h, stream)

    def log(self, stream):
        buf = C.create_string_buffer(1 << 16)
        _need(lib().dabhip_multi_stream_log(self._h, stream, buf, len(buf)) >= 0, "multi_stream_log")
        return buf.value.decode("ascii")

    def eti(self, stream):
        n = lib().dabhip_multi_eti_count(self._h, stream)
        _need(n >= 0, "multi_eti_count")
        out = np.zeros((n, ETI_BYTES), dtype=np.uint8)
        if n:
            _need(lib().dabhip_multi_eti_read(self._h, stream, _p(out), n) == n, "multi_eti_read")
        return out

    def drain(self):
        """All frames through dabhip_multi_eti_drain -> [(stream, frame bytes)] in emission order."""
        got = []
        sink = C.CFUNCTYPE(None, u8p, C.c_int, C.c_void_p)(lambda p, b, _u: got.append((b, C.string_at(p, ETI_BYTES))))      # (not numpy's as_array: it holds on to ~100 bytes per distinct address)
        n = lib().dabhip_multi_eti_drain(self._h, C.cast(sink, C.c_void_p), None)
        _need(n == len(got), "multi_eti_drain")
        return got

    def trace(self, stream, ncalls):
        ints = np.zeros((ncalls, 6), dtype=np.int32)
        ffs = np.zeros(ncalls, dtype=np.float64)
        n = lib().dabhip_multi_trace(self._h, stream, ints.ctypes.data_as(C.POINTER(C.c_int32)), ffs.ctypes.data_as(C.POINTER(C.c_double)), ncalls)
        _need(n >= 0, "multi_trace")
        return ints[:n], ffs[:n]

    def engine(self, slice_index):
        """The slice's engine (borrowed: stage_ms(), guard_stats(), ...)."""
        h = lib().dabhip_multi_engine(self._h, slice_index)
        _need(h, "multi_engine")
        return Engine(_borrowed=h)

    def wall_ms(self, slice_index=-1):
        return lib().dabhip_multi_wall_ms(self._h, slice_index)


class Stream(_Handle):
    """Streaming session (dabhip_stream_*): B unbounded captures decoded segment by segment; the concatenated ETI
    frames equal one Engine.decode of the whole captures."""

    _PREFIX, _destroy = "dabhip_stream_", "dabhip_stream_destroy"
    _RENAMED = {}

    def _f(self, name):
        return getattr(lib(), self._PREFIX + self._RENAMED.get(name, name))

    def __init__(self, nstreams, device=0, afc=False, soft=False, subchannels=None, guard=None):
        self._h = lib().dabhip_stream_create(device, nstreams)
        _need(self._h, "stream_create")
        self.nstreams = nstreams
        self._configure(afc, soft, subchannels, guard)

    def _configure(self, afc, soft, subchannels, guard):
        if subchannels:
            ids = list(subchannels)
            _need(self._f("set_subchannels")(self._h, (C.c_int32 * len(ids))(*ids), len(ids)) == 0, "stream_set_subchannels")
        if afc:
            _need(self._f("set_afc")(self._h, 1) == 0, "stream_set_afc")
        if soft:
            _need(self._f("set_soft")(self._h, 1) == 0, "stream_set_soft")
        if guard is not None:
            self.set_parity_guard(guard)

    def set_parity_guard(self, level=True):
        """see Engine.set_parity_guard"""
        _need(self._f("set_parity_guard")(self._h, _guard_level(level)) == 0, "stream_set_parity_guard")

    def set_soft_lanes(self, enable):
        """see Engine.set_soft_lanes (any time; single- and multi-device sessions)"""
        _need(self._f("set_soft_lanes")(self._h, 1 if enable else 0) == 0, "stream_set_soft_lanes")

    def set_tii(self, enable):
        """see Engine.set_tii: the sums accumulate over the session's segments until tii_reset (single-device sessions)"""
        self._single_device("set_tii")
        _need(lib().dabhip_stream_set_tii(self._h, 1 if enable else 0) == 0, "stream_set_tii")

    def tii_sums(self, stream):
        self._single_device("tii_sums")
        return _tii_sums(lib().dabhip_stream_tii_sums, self._h, stream)

    def tii(self, stream):
        self._single_device("tii")
        return _tii_ids(lib().dabhip_stream_tii, self._h, stream)

    def tii_reset(self):
        self._single_device("tii_reset")
        _need(lib().dabhip_stream_tii_reset(self._h) == 0, "stream_tii_reset")

    def _single_device(self, what):
        """The entries that exist for dabhip_stream handles only: a multi-device session's handle is another type."""
        if self._PREFIX != "dabhip_stream_":
            raise DabhipError("%s: single-device sessions only" % what)

    def set_demod_all(self, on):
        """see Engine.set_demod_all (single-device sessions)"""
        self._single_device("set_demod_all")
        _need(lib().dabhip_stream_set_demod_all(self._h, 1 if on else 0) == 0, "stream_set_demod_all")

    def msc_deferred(self):
        """TFs of the segment fed last whose MSC symbols were deferred by the lock-in skip (single-device sessions)."""
        self._single_device("msc_deferred")
        n = lib().dabhip_stream_msc_deferred(self._h)
        _need(n >= 0, "stream_msc_deferred")
        return n

    def set_launch_limits(self, **limits):
        """see Engine.set_launch_limits (single-device sessions)"""
        self._single_device("set_launch_limits")
        _set_launch_limits(lib().dabhip_stream_set_launch_limits, self._h, limits)

    def launch_report(self):
        """The launches of the segment fed last, its device gathers included (see Engine.launch_report; single-device sessions)."""
        self._single_device("launch_report")
        return _launch_report(lib().dabhip_stream_launch_report, self._h)

    def log(self, stream):
        """The reference's operator messages for one stream since the last call (dabhip_stream_log): 'Locked', 'Lock lost, resetting ringbuffer', ensemble dump."""
        buf = C.create_string_buffer(1 << 16)
        n = self._f("log")(self._h, stream, buf, len(buf))
        _need(n >= 0, "stream_log")
        return buf.value.decode("ascii")

    def feed(self, segments):
        """segments: one numpy uint8 array (possibly empty) per stream -> ETI frames produced by this segment."""
        arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in segments]
        _need(len(arrs) == self.nstreams, "stream_feed: one segment per stream")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        n = self._f("feed")(self._h, ptrs, sizes, 0)
        _need(n >= 0, "stream_feed")
        return n

    def feed_ptrs(self, ptrs, sizes, on_device=False):
        """feed() over raw addresses (page-locked host memory from host_alloc(), or device memory)."""
        p = (C.c_void_p * len(ptrs))(*ptrs)
        s = (C.c_size_t * len(sizes))(*sizes)
        n = self._f("feed")(self._h, p, s, 1 if on_device else 0)
        _need(n >= 0, "stream_feed")
        return n

    def feed_resident(self, base_ptrs, avail):
        """dabhip_stream_feed_resident: the streams live in device memory (base_ptrs[b] + x = byte x of stream b) and are read in place;
        avail[b] = bytes there now."""
        p = (C.c_void_p * len(base_ptrs))(*base_ptrs)
        a = (C.c_size_t * len(avail))(*avail)
        n = self._f("feed_resident")(self._h, p, a)
        _need(n >= 0, "stream_feed_resident")
        return n

    def need_from(self, stream):
        return int(self._f("need_from")(self._h, stream))

    def prefetch_ptrs(self, ptrs, sizes, on_device=False):
        """dabhip_stream_prefetch: start uploading the segment a later feed_ptrs() with the same arguments will consume."""
        p = (C.c_void_p * len(ptrs))(*ptrs)
        s = (C.c_size_t * len(sizes))(*sizes)
        _need(self._f("prefetch")(self._h, p, s, 1 if on_device else 0) == 0, "stream_prefetch")

    def status(self, stream):
        return int(self._f("status")(self._h, stream))

    def set_sync_speculation(self, mode):
        """see Engine.set_sync_speculation"""
        _need(self._f("set_sync_speculation")(self._h, int(mode)) == 0, "stream_set_sync_speculation")

    def stage_ms(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = lib().dabhip_stream_stage_ms(self._h, names, ms, 16)
        return {names[i].decode(): ms[i] for i in range(n)}

    def eti_fetch(self, dst_ptr, cap_frames):
        """dabhip_stream_eti_fetch: all frames of the segment fed last on their way to (page-locked) host memory; returns their number."""
        n = self._f("eti_fetch")(self._h, dst_ptr, cap_frames)
        _need(n >= 0, "stream_eti_fetch")
        return n

    def eti_fetch_wait(self):
        _need(self._f("eti_fetch_wait")(self._h) == 0, "stream_eti_fetch_wait")

    def eti_count(self, stream):
        return int(self._f("eti_count")(self._h, stream))

    def eti(self, stream):
        n = self._f("eti_count")(self._h, stream)
        _need(n >= 0, "stream_eti_count")
        out = np.zeros((n, ETI_BYTES), dtype=np.uint8)
        if n:
            _need(self._f("eti_read")(self._h, stream, _p(out), n) == n, "stream_eti_read")
        return out


class MultiStream(Stream):
    """Sessions over several devices (dabhip_multi_stream_*): nstreams unbounded captures dealt ONCE to the listed devices in contiguous slices (the rule
    of Multi.plan), every slice a complete Stream session on its device; every call is made on all slices at once.  Frames per segment and in total are
    those of one Stream over all captures.  A device may be listed several times (every entry is its own slice)."""
    _PREFIX, _destroy = "dabhip_multi_stream_", "dabhip_multi_stream_destroy"
    _RENAMED = {"status": "status_of", "log": "log_of"}

    def __init__(self, nstreams, devices, afc=False, soft=False, subchannels=None, guard=None):
        devs = list(devices)
        self._h = lib().dabhip_multi_stream_create((C.c_int * len(devs))(*devs), len(devs), nstreams)
        _need(self._h, "multi_stream_create")
        self.nstreams = nstreams
        self.devices = devs
        self._configure(afc, soft, subchannels, guard)

    def slice_of(self, stream):
        """(slice, device, first stream of the slice, streams in the slice)"""
        dev, first, count = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        sl = lib().dabhip_multi_stream_slice_of(self._h, stream, C.byref(dev), C.byref(first), C.byref(count))
        _need(sl >= 0, "multi_stream_slice_of")
        return sl, dev.value, first.value, count.value

    def stage_ms(self, slice_index=0):
        h = lib().dabhip_multi_stream_session(self._h, slice_index)
        _need(h, "multi_stream_session")
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = lib().dabhip_stream_stage_ms(h, names, ms, 16)
        return {names[i].decode(): ms[i] for i in range(n)}
