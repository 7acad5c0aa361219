#!/usr/bin/env python3
"""tools/models/multilane_soft_model.py -- the SOFT decoder with 2^NL lanes per code word (NL = 1, 2): vit_soft_lanes.hpp on the CPU.

multilane_model.py's lane-bit rotation (places (3 + t) mod 6 and (5 + t) mod 6 beside the pair bit t mod 4), compaction numbering and exchange, with what
soft values change:
  * metrics x16 with four tag bits, so a block is 4 steps and every re-pairing clears the tags; the rotation has period 6, so blocks come in three
    variants (lane places (3, 5), (1, 3), (5, 1) at the start of block b for b mod 3 = 0, 1, 2);
  * branch metrics from the lane form's ONE pair of tables (k_decode.hip: build_soft_lut; a -8 counts as -7 inside the table): the eight packed words
    W(c), c < 4 the sum of the two rows, W(c ^ 7) = kAll - W(c), are indexed by c ^ g, g = the lane's code offset = XOR of code(2 << L_i) over its set lane
    bits below place 5 -- every lane reads the rows of the values AS RECEIVED, so no sign is flipped and -8 needs no special case;
  * at an exchange over lane bit i the lanes with that bit set own the high predecessor: the tag goes to the partner's words instead of their own;
  * half-records: a lane's tag nibbles after a block, register R -> word R >> 2, byte 2 (R & 1) + half, high nibble for R & 2; two of them per unit
    of 8 steps; the last 1..3 steps of a code word leave a half-record of which only state 0's nibble is read;
  * chain-back from state 0 over the half-records, inverting the compaction numbering of the layout at each block's end (pair bit 4).
decode() returns the decoded bytes before the energy-dispersal XOR; decode_one_lane() is the plain 64-state decoder with the same metric and tie
rule (the high predecessor wins only when strictly better).  run() also asserts the lanes' registers against the 64 plain metrics after every step.
Usage: multilane_soft_model.py [steps=774]"""
import random
import sys

SHIFT = 4
K_ALL = 56 << SHIFT
K_BASE = 8192
REBASE_STEPS = 32


def parity(x):
    return bin(x).count("1") & 1


def code3(i):
    return parity(i & 0x6d) | (parity(i & 0x4f) << 1) | (parity(i & 0x53) << 2)


def compact(k, removed):
    out, pos = 0, 0
    for b in range(6):
        if b in removed:
            continue
        out |= ((k >> b) & 1) << pos
        pos += 1
    return out


def expand(P, removed):
    out, pos = 0, 0
    for b in range(6):
        if b in removed:
            continue
        out |= ((P >> pos) & 1) << b
        pos += 1
    return out


def places(NL, t):
    return tuple((a + t) % 6 for a in (3, 5)[:NL])


def lane_of(k, Ls):
    return sum(((k >> L) & 1) << i for i, L in enumerate(Ls))


def clamp(s):
    return max(s, -7)


def lut_words(values, tau):
    """the step's four packed words (lo: code c, hi: code c ^ gamma(tau)) for c = 0..3: row of table a (s0, s3) + row of table b (s1, s2)"""
    s0, s1, s2, s3 = (clamp(v) for v in values)
    gamma = code3(2 << tau)

    def part_a(code):
        q = code if code < 4 else code ^ 7
        share = 14 + (-1 if q & 1 else 1) * (s0 + s3)
        return (share if code < 4 else 28 - share) << SHIFT

    def part_b(code):
        q = code if code < 4 else code ^ 7
        share = 14 + (-1 if q & 2 else 1) * s1 + s2
        return (share if code < 4 else 28 - share) << SHIFT

    return [(part_a(c) + part_b(c), part_a(c ^ gamma) + part_b(c ^ gamma)) for c in range(4)]


def plain_metrics(values):
    """metric of code c = (28 + sum_j sigma_cj s_j) << 4: bit 0 of c flips s0 and s3, bit 1 s1, bit 2 s2"""
    s0, s1, s2, s3 = (clamp(v) for v in values)
    bm = []
    for c in range(8):
        bm.append((28 + (-1 if c & 1 else 1) * (s0 + s3) + (-1 if c & 2 else 1) * s1 + (-1 if c & 4 else 1) * s2) << SHIFT)
    return bm


def pack_bits(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        out[i >> 3] |= b << (7 - (i & 7))
    return bytes(out)


def decode_one_lane(values, nsteps):
    """plain 64-state add-compare-select and chain-back from state 0; values: 4 per step (0 = not received)"""
    M = [0] * 64
    M[0] = K_BASE
    dec = []
    for t in range(nsteps):
        bm = plain_metrics(values[4 * t:4 * t + 4])
        new, d = [0] * 64, [0] * 64
        for j in range(32):
            c = code3(2 * j)
            for odd in (0, 1):
                m0, m1 = M[j] + bm[c ^ (7 * odd)], M[j + 32] + bm[c ^ 7 ^ (7 * odd)]
                d[2 * j + odd] = int(m1 > m0)
                new[2 * j + odd] = max(m0, m1)
        M = new
        dec.append(d)
    state, bits = 0, [0] * (nsteps - 6)
    for t in range(nsteps - 1, 5, -1):
        bit = dec[t][state]
        bits[t - 6] = bit
        state = (state | (bit << 6)) >> 1
    return pack_bits(bits)


def add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def vmax(a, b):
    return (max(a[0], b[0]), max(a[1], b[1]))


def pack_half_record(regs):
    """a lane's registers -> nreg / 4 words of tag nibbles"""
    words = [0] * (len(regs) // 4)
    for R, (lo, hi) in enumerate(regs):
        for half, x in ((0, lo), (1, hi)):
            words[R >> 2] |= (x & 15) << (8 * (2 * (R & 1) + half) + 4 * ((R >> 1) & 1))
    return words


def decode(values, nsteps, NL, check=False):
    """the multi-lane decoder; returns the decoded bytes.  check: assert the registers against the plain metrics after every step"""
    nlanes, nreg = 1 << NL, 1 << (5 - NL)
    assert nsteps % 8 in (0, 4, 5, 6, 7), "a code word ends in a unit's second block or at a block's end"
    regs = [[(0, 0)] * nreg for _ in range(nlanes)]
    regs[0][0] = (K_BASE, 0)
    M = [0] * 64
    M[0] = K_BASE
    records = []                                           # [block][lane] -> words
    tau = 0
    for t in range(nsteps):
        Ls, Ln = places(NL, t), places(NL, t + 1)
        assert tau == t % 4 and tau not in Ls and len(set(Ls)) == NL
        vals = values[4 * t:4 * t + 4]
        tag = 1 << tau
        w = lut_words(vals, tau)
        W = [None] * 8
        for c in range(4):
            W[c] = w[c]
            W[c ^ 7] = (K_ALL - w[c][0], K_ALL - w[c][1])
        gamma = code3(2 << tau)
        bm = plain_metrics(vals)
        for c in range(8):
            assert W[c] == (bm[c], bm[c ^ gamma]), (t, c)
        if check:
            Mn = [0] * 64
            for j in range(32):
                c = code3(2 * j)
                Mn[2 * j] = max(M[j] + bm[c] + tag, M[j + 32] + bm[c ^ 7])
                Mn[2 * j + 1] = max(M[j] + bm[c ^ 7] + tag, M[j + 32] + bm[c])
        at5 = [i for i, L in enumerate(Ls) if L == 5]
        new = [[None] * nreg for _ in range(nlanes)]
        for lane in range(nlanes):
            Wl = list(W)
            for i, L in enumerate(Ls):                     # one level of selects per lane bit below place 5
                if L < 5 and (lane >> i) & 1:
                    g = code3(2 << L)
                    Wl = [Wl[c ^ g] for c in range(8)]
            p = regs[lane]
            removed_in, removed_out = set(Ls) | {tau}, set(Ln) | {tau + 1}
            if at5:
                i5 = at5[0]
                high = (lane >> i5) & 1
                A = [(x[0] + (0 if high else tag), x[1] + (0 if high else tag)) for x in Wl]
                B = [(x[0] + (tag if high else 0), x[1] + (tag if high else 0)) for x in Wl]
                partner = regs[lane ^ (1 << i5)]
                for r in range(nreg):
                    j = expand(r, removed_in)
                    c = code3(2 * j)
                    P = compact(2 * j, removed_out)
                    assert new[lane][P] is None
                    new[lane][P] = vmax(add(p[r], A[c]), add(partner[r], B[c ^ 7]))
            else:
                A = [(x[0] + tag, x[1] + tag) for x in Wl]
                B = Wl
                for q in range(nreg // 2):
                    j0 = expand(q, removed_in)
                    assert j0 < 32 and expand(q + nreg // 2, removed_in) == j0 + 32
                    c = code3(2 * j0)
                    x, y = p[q], p[q + nreg // 2]
                    Pe, Po = compact(2 * j0, removed_out), compact(2 * j0 + 1, removed_out)
                    assert new[lane][Pe] is None and new[lane][Po] is None and Pe != Po
                    new[lane][Pe] = vmax(add(x, A[c]), add(y, B[c ^ 7]))
                    new[lane][Po] = vmax(add(x, A[c ^ 7]), add(y, B[c]))
        regs, tau = new, tau + 1
        if check:
            M = Mn
            for k in range(64):
                assert regs[lane_of(k, Ln)][compact(k, set(Ln) | {tau})][(k >> tau) & 1] == M[k], (t, k)
        last = t == nsteps - 1
        if tau == 4 or last:
            records.append([pack_half_record(regs[lane]) for lane in range(nlanes)])
            if last and tau < 4:
                assert lane_of(0, Ln) == 0 and compact(0, set(Ln) | {tau}) == 0     # state 0: lane 0, register 0, low half
        if tau == 4:                                       # re-pair inside each lane, tags cleared
            new = [[None] * nreg for _ in range(nlanes)]
            for lane in range(nlanes):
                for P in range(nreg):
                    k = expand(P, set(Ln) | {0})
                    for i, L in enumerate(Ln):
                        k |= ((lane >> i) & 1) << L
                    a, b, half = compact(k, set(Ln) | {4}), compact(k + 1, set(Ln) | {4}), (k >> 4) & 1
                    new[lane][P] = (regs[lane][a][half] & ~15, regs[lane][b][half] & ~15)
            regs, tau = new, 0
            M = [x & ~15 for x in M]
        if (t + 1) % REBASE_STEPS == 0 and not last:
            assert tau == 0
            base = regs[0][0][0] - K_BASE
            regs = [[(a - base, b - base) for a, b in lane] for lane in regs]
            M = [x - base for x in M]
            assert all(0 <= a < 65536 and 0 <= b < 65536 for lane in regs for a, b in lane)
    # chain-back in one lane over the lanes' half-records
    nfull, r = nsteps >> 2, nsteps & 3
    state, bits = 0, [0] * (nsteps - 6)

    def consume(nib, t0, k_hi):
        nonlocal state
        for k in range(3, -1, -1):
            t = t0 + k
            if k <= k_hi and t >= 6:
                bit = ((nib >> k) & 1) ^ 1
                state = (state | (bit << 6)) >> 1
                bits[t - 6] = bit

    if r:
        consume(records[nfull][0][0] & 15, 4 * nfull, r - 1)
    for b in range(nfull - 1, 0, -1):
        m3 = (b + 1) % 3
        Ls = ((3, 5), (1, 3), (5, 1))[m3][:NL]
        assert Ls == places(NL, 4 * (b + 1))
        lane, P, half = lane_of(state, Ls), compact(state, set(Ls) | {4}), (state >> 4) & 1
        shift = 8 * (2 * (P & 1) + half) + 4 * ((P >> 1) & 1)
        consume((records[b][lane][P >> 2] >> shift) & 15, 4 * b, 3)
    return pack_bits(bits)


def random_values(rnd, nsteps, lo=-7, hi=7):
    """random received values with a random number 0..4 of values per step (the first n of four, as the puncturing keeps them)"""
    out = []
    for _ in range(nsteps):
        n = rnd.randrange(5)
        out += [rnd.randint(lo, hi) if j < n else 0 for j in range(4)]
    return out


def run(NL, nsteps, seed, lo=-7, hi=7):
    rnd = random.Random(seed)
    values = random_values(rnd, nsteps, lo, hi)
    assert decode(values, nsteps, NL, check=True) == decode_one_lane(values, nsteps)
    return True


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 774
    for NL in (1, 2):
        run(NL, steps, 17 + NL)
        run(NL, steps, 27 + NL, -8, 7)
        run(NL, steps, 37 + NL, -1, 1)
        print("%d lanes per code word: %d steps equal to the plain 64-state soft decoder (values -7..7, -8..7, -1..1)" % (1 << NL, steps))


if __name__ == "__main__":
    main()
