"""EEP sub-channels of every size: the shapes tests/test_gpu_eep_sizes.py decodes, packed into ensembles.  Test infrastructure.

An item is (slform = 1, level, size_cu): level 0 .. 3 = protection 1-A .. 4-A (a unit n is 8 kbit/s, 24 bytes and 192 data bits per CIF), 4 .. 7 = 1-B .. 4-B
(32 kbit/s, 96 bytes, 768 bits).  Two lists of ensembles, each ensemble a list of (slform, level, size_cu, start_cu) as _profile_ensembles of
test_gpu_parity_r2.py makes them:

  REF     every code word has at most 13,824 data bits, the length the reference's own decoder is created for (dab.c:29): checked against the real back end
          AND the oracle.  1-A .. 4-A at n = 3, 5 (odd, the smallest untested), 6, 9, 12 (the DAB+ service sizes), 24 and 72 (the reference's capacity; at
          1-A a whole CIF); 1-B .. 4-B at n = 3, 6 and 18 (the reference's capacity).
  ORACLE  beyond it, checked against the oracle, whose decoder allocates by length: the largest n that fits 864 CU at each level (2-A 108, 3-A 144, 4-A 216,
          1-B 32, 2-B 41, 3-B 48, 4-B 57: WHOLE_CIF); 4-A at n = 170 / 171 and 4-B at n = 42 / 43, the last sub-channel of at most 4,096 bytes per CIF and
          the first above (4,080 / 4,104 and 4,032 / 4,128 bytes: the decoders' descrambling table once ended there); 4-A at n = 73 and 4-B at n = 19, one past
          the reference's capacity.  Each has an ensemble of its own, its free CUs filled FROM THE FRONT with small REF shapes: the table-edge and past-REF
          shapes start at CU 180 .. 270.  The whole-CIF shapes leave 0 to 9 CU, less than the smallest filler's 12, and start at CU 0 here (a whole-CIF
          code word at another start address: the 4-B n = 57 capture of test_gpu_eep_sizes.py, CU 9).

What a multiplex must satisfy is restated here from layout_fault (control_plane.hpp) and asserted for every ensemble; nothing is skipped."""

CU_PER_UNIT = [12, 8, 6, 4, 27, 21, 18, 15]            # CUs of one unit n at level 0 .. 7 (ETSI EN 300 401 11.3.2; dab_tables.c:98-127)
LEVEL_NAMES = ["1-A", "2-A", "3-A", "4-A", "1-B", "2-B", "3-B", "4-B"]
REF_MAX_BITS = 768 * 18                                 # create_viterbi(768*18), dab.c:29
OLD_TABLE_BYTES = 4096

REF_N_A = (3, 5, 6, 9, 12, 24, 72)
REF_N_B = (3, 6, 18)
WHOLE_CIF = [(1, 108), (2, 144), (3, 216), (4, 32), (5, 41), (6, 48), (7, 57)]          # (level, n)
TABLE_EDGE = [(3, 170), (3, 171), (7, 42), (7, 43)]
PAST_REF = [(3, 73), (7, 19)]


def item(level, n):
    return (1, level, CU_PER_UNIT[level] * n)


def units(it):
    return it[2] // CU_PER_UNIT[it[1]]


def bytes_per_cif(it):
    """Decoded bytes of the sub-channel in one ETI frame: bit rate x 24 ms."""
    return units(it) * (24 if it[1] < 4 else 96)


def data_bits(it):
    return 8 * bytes_per_cif(it)


def name(it):
    return "EEP %s n=%d" % (LEVEL_NAMES[it[1]], units(it))


REF_ITEMS = [item(lev, n) for lev in range(4) for n in REF_N_A] + [item(lev, n) for lev in range(4, 8) for n in REF_N_B]
ORACLE_ITEMS = [item(lev, n) for lev, n in WHOLE_CIF + TABLE_EDGE + PAST_REF]
WHOLE_CIF_ITEMS = [item(lev, n) for lev, n in WHOLE_CIF]
# what fills the free CUs of a large item's ensemble: the small REF shapes
FILLERS = [item(lev, n) for n in (3, 5, 6) for lev in range(4)] + [item(lev, 3) for lev in range(4, 8)]


def configure(ei, ens):
    """The modulator's configuration of ensemble number ei (seed, CIF counter and SubChIds follow from it): the rule of test_gpu_decoder_forms.py's
    _profile_cfg, restated here so that the CPU test of this module imports no GPU test."""
    import dabtools_amd as dab
    cfg = dab.synth_preset(1, seed=900 + ei, cif_count0=240 + ei)
    cfg.nsub = len(ens)
    for k, (slform, idx, size, start) in enumerate(ens):
        s = cfg.sub[k]
        s.id = (7 * k + ei) % 64 if len(ens) <= 9 else k * 3
        s.start_cu, s.slform, s.size_cu = start, slform, size
        s.uep_index = idx if slform == 0 else 0
        s.eep_protlev = idx if slform == 1 else 0
    assert len({cfg.sub[k].id for k in range(cfg.nsub)}) == cfg.nsub
    return cfg


def _pack(items):
    """Largest first into ensembles of at most 864 CU and 18 sub-channels (as _profile_ensembles does)."""
    ensembles, cur, cu = [], [], 0
    for it in sorted(items, key=lambda x: -x[2]):
        if cu + it[2] > 864 or len(cur) == 18:
            ensembles.append(cur)
            cur, cu = [], 0
        cur.append(it + (cu,))
        cu += it[2]
    ensembles.append(cur)
    return ensembles


def frame_bytes(ens):
    """ETI bytes of the multiplex as layout_fault counts them: header (8 + 4 nst + 4), 96 of FIC, each sub-channel's bytes rounded up to 8, EOF + TIST."""
    return 8 + 4 * len(ens) + 4 + 96 + sum((bytes_per_cif(it) + 7) & ~7 for it in ens) + 8


def check_layout(ens):
    """layout_fault's rules (and no two sub-channels on one CU, which the modulator needs)."""
    used = set()
    for it in ens:
        slform, level, size, start = it
        assert slform == 1 and 0 <= level < 8 and size >= CU_PER_UNIT[level] and size % CU_PER_UNIT[level] == 0, it
        assert start >= 0 and start + size <= 864, (name(it), start)
        cus = set(range(start, start + size))
        assert not (used & cus), (name(it), start)
        used |= cus
    assert frame_bytes(ens) <= 6144, (frame_bytes(ens), [name(it) for it in ens])
    assert len(ens) <= 64


def ensembles():
    """-> (REF ensembles, ORACLE ensembles)"""
    ref = _pack(REF_ITEMS)
    oracle = []
    for k, big in enumerate(ORACLE_ITEMS):
        free, front = 864 - big[2], []
        # first fit over the fillers, from a place that moves with k so that the large items meet different neighbours; at most 6 of them
        for j in range(len(FILLERS)):
            f = FILLERS[(j + 3 * k) % len(FILLERS)]
            if f[2] <= free and len(front) < 6 and frame_bytes([big] + front + [f]) <= 6144:
                front.append(f)
                free -= f[2]
        ens, cu = [], 0
        for it in front + [big]:
            ens.append(it + (cu,))
            cu += it[2]
        oracle.append(ens)
    # ---- what the lists promise -----------------------------------------------------------------------------------------------------
    covered_ref = {it[:3] for ens in ref for it in ens}
    covered_or = {it[:3] for ens in oracle for it in ens}
    assert covered_ref == set(REF_ITEMS) and len(REF_ITEMS) == 4 * 7 + 4 * 3
    assert set(ORACLE_ITEMS) <= covered_or and covered_or <= set(ORACLE_ITEMS) | set(FILLERS) and len(set(ORACLE_ITEMS)) == 13
    for ens in ref + oracle:
        check_layout(ens)
    assert all(data_bits(it) <= REF_MAX_BITS for ens in ref for it in ens)
    assert all(data_bits(it) > REF_MAX_BITS for it in ORACLE_ITEMS)
    assert max(data_bits(it) for it in REF_ITEMS) == REF_MAX_BITS                      # n = 72 at A, n = 18 at B: exactly the reference's capacity
    assert [bytes_per_cif(item(lev, n)) for lev, n in TABLE_EDGE] == [4080, 4104, 4032, 4128]
    assert all(864 - CU_PER_UNIT[it[1]] < it[2] <= 864 for it in WHOLE_CIF_ITEMS)          # one more unit would not fit the CIF
    assert any(ens[-1][3] > 0 for ens in oracle) and len(ref) <= 10
    return ref, oracle


def above_old_table(ens):
    """Does the ensemble hold a sub-channel of more than 4,096 bytes per CIF?"""
    return any(bytes_per_cif(it) > OLD_TABLE_BYTES for it in ens)
