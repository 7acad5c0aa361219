"""tests/eep_sizes.py without a GPU: the packing keeps its promises, and the product's own control plane (layout_fault, control_plane.hpp) accepts every
ensemble -- 16 TFs of its FIBs give the 12 frame jobs the GPU tests expect -- while a sub-channel that ends past the CIF by one unit or a few CUs gives none
(EEP sub-channels that do not overlap carry at most 6.4 bytes per CU, 5,530 bytes per CIF: such a multiplex cannot overflow the ETI frame)."""
import numpy as np
import pytest

import dabtools_amd as dab
import eep_sizes as sizes


def _jobs(ei, ens, ntf=16):
    cfg = sizes.configure(ei, ens)
    fibs = np.stack([np.concatenate([dab.synth_fibs(cfg, 4 * t + q) for q in range(4)]) for t in range(ntf)])
    first, headers = dab.host_control_replay(fibs, np.ones((ntf, 12), np.uint8))
    return len(first), headers


def test_every_ensemble_is_one_the_control_plane_accepts():
    ref, oracle = sizes.ensembles()
    assert 8 <= len(ref) <= 10 and len(oracle) == 13
    for ei, ens in enumerate(ref + oracle):
        n, headers = _jobs(ei, ens)
        assert n == 12, [sizes.name(it) for it in ens]
        assert (headers[0][5] & 0x7f) == len(ens)
    # the largest code word is the one the issue names
    assert max(sizes.data_bits(it) for ens in oracle for it in ens) + 6 == 43782
    assert max(sizes.bytes_per_cif(it) for ens in oracle for it in ens) == 5472 <= dab.ETI_BYTES


@pytest.mark.parametrize("level,n,start", [(3, 217, 0), (7, 58, 0), (3, 216, 1), (7, 57, 10)])
def test_a_subchannel_past_the_cif_is_refused(level, n, start):
    assert _jobs(50, [(1, level, sizes.CU_PER_UNIT[level] * n, start)])[0] == 0


def test_synth_payload_reaches_the_largest_subchannel():
    for level, n in sizes.WHOLE_CIF:
        cfg = sizes.configure(60 + level, [sizes.item(level, n) + (0,)])
        assert dab.synth_payload(cfg, 7, 0).size == sizes.bytes_per_cif(sizes.item(level, n))
