"""The multiplexes and filters that tests/test_eti_filter_model.py (CPU) and tests/test_gpu_subch_filter.py (GPU) share.  Test infrastructure; imports no
GPU test."""
import eep_sizes

DENSE_IDS = [3 * k + 1 for k in range(20)]
DENSE_SMALLEST, DENSE_LARGEST = 19, 46          # EEP 1-A n = 1 (24 bytes per CIF) and EEP 4-A n = 16 (384 bytes): held by the CPU test against the oracle's STL
DENSE_FILTERS = {
    "smallest": [DENSE_SMALLEST],
    "largest": [DENSE_LARGEST],
    "every-second": DENSE_IDS[::2],
    "all-but-one": [i for i in DENSE_IDS if i != 28],
    "first-and-last": [DENSE_IDS[0], DENSE_IDS[-1]],
}


def dense_cfg(seed, snr=1000.0, skip=0):
    """The 20-sub-channel multiplex of test_gpu_parity.test_engine_many_subchannels_and_uep_eep_mix (6 UEP, 14 EEP, SubChIds 1, 4, .. 58)."""
    import dabtools_amd as dab
    cfg = dab.synth_preset(0, seed=seed, snr_db=snr, cif_count0=(31 * seed) % 5000, skip_samples=skip)
    cfg.nsub = 0
    cu = 0
    uep_cu = [16, 21, 24, 29, 35, 24, 29, 35, 42, 52, 29, 35, 42, 52, 32, 42, 48, 58, 70, 40]
    for slform, idx, size in [(0, i, 0) for i in (0, 4, 5, 9, 14, 18)] + \
            [(1, lev, size) for lev, size in ((0, 12), (1, 8), (2, 6), (3, 4), (4, 27), (5, 21), (6, 18), (7, 15), (0, 96), (3, 64), (1, 16), (2, 12), (3, 8), (7, 30))]:
        s = cfg.sub[cfg.nsub]
        s.id, s.start_cu, s.slform = DENSE_IDS[cfg.nsub], cu, slform
        if slform == 0:
            s.uep_index = idx
            cu += uep_cu[idx]
        else:
            s.eep_protlev, s.size_cu = idx, size
            cu += size
        cfg.nsub += 1
    assert cfg.nsub == 20 and cu <= 864
    return cfg


def _eep_cfg(seed, cif_count0, subs):
    """subs: [(SubChId, level, n units)] laid one behind the other from CU 3 on."""
    import dabtools_amd as dab
    cfg = dab.synth_preset(1, seed=seed, cif_count0=cif_count0)
    cfg.nsub, cu, ens = len(subs), 3, []
    for k, (sid, level, n) in enumerate(subs):
        it = eep_sizes.item(level, n)
        s = cfg.sub[k]
        s.id, s.start_cu, s.slform, s.uep_index, s.eep_protlev, s.size_cu = sid, cu, 1, 0, level, it[2]
        ens.append(it + (cu,))
        cu += it[2]
    eep_sizes.check_layout(ens)
    return cfg


EDGE_IDS = [0, 31, 32, 63]
EDGE_FILTERS = [[0], [63], [31, 32], [63, 63, 0], [64], [-1, 1000], []]


def edge_cfg(seed=7301):
    """Sub-channels at the ends of the 64-bit mask and on both sides of its 32-bit middle."""
    return _eep_cfg(seed, 246, [(0, 2, 5), (31, 0, 3), (32, 5, 3), (63, 3, 9)])


LARGE_ID, LARGE_SMALL_IDS = 30, [7, 12, 44, 51]
LARGE_FILTERS = {"large-only": [LARGE_ID], "small-only": LARGE_SMALL_IDS, "large-and-last-small": [LARGE_ID, LARGE_SMALL_IDS[-1]]}


def large_cfg(seed=7302):
    """EEP 3-A n = 72 (13,824 data bits, the longest code word the reference decodes; 1,728 bytes per CIF) from CU 47 on, two small sub-channels in front
    of it and two behind: unfiltered its bytes start 192 bytes behind the FIC, kept alone right behind it, and the last small one follows it or not."""
    cfg = _eep_cfg(seed, 4990, [(7, 1, 3), (12, 3, 5), (LARGE_ID, 2, 72), (44, 0, 3), (51, 6, 3)])
    assert cfg.sub[2].start_cu == 3 + 24 + 20 and eep_sizes.data_bits(eep_sizes.item(2, 72)) == eep_sizes.REF_MAX_BITS
    return cfg
