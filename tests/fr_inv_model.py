"""TEST SUPPORT (no kernel code): the device form of the field inversion, fr_dev.hpp fr_inv_kaliski_inl, restated on Python ints.

Kaliski's almost-inverse with batched shifts, as the wavefront runs it: the lanes of a wave (up to 64) go through the loop in lock-step,
`__any` is any() over the wave, an even-fix iteration is taken by EVERY lane as soon as one lane needs it (the others shift by 0), and the
wave leaves the loop when no lane is active.  Per lane the model returns the Montgomery result, k and counters of the branches the lane
took; per wave the number of loop iterations.  What the code's comments claim is asserted on the way: r + s, s << t and r << t stay below
2^256 (the C code drops the carry), r < 2p at the end, the loop ends by itself within its bound, and k indexes the table.

Phase 2 multiplies by 2^(768-k) mod p computed here; that fr_pow2_table.h holds the same numbers is a test of its own."""
from dataclasses import dataclass, field

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R = 2 ** 256 % P
RINV = pow(R, P - 2, P)
M32 = 0xFFFFFFFF
LOOP_BOUND = 1100                 # fr_dev.hpp: for (int it = 0; it < 1100; it++)
POW2_TAB_LEN = 521                # fr_pow2_table.h FR_POW2_TAB_LEN


@dataclass
class Lane:
    result: int = 0               # Montgomery form: x^-1 * 2^512 mod p for the input x (= a * 2^256), 0 for 0
    k: int = 0
    even_fix: int = 0             # even-fix steps in which this lane had a value to shift
    even_fix_w0_zero: int = 0     # ... whose low limb was 0 (shift 31)
    both_odd: int = 0             # both-odd steps this lane took while active
    both_odd_d0_zero: int = 0     # ... with d[0] == 0 and d != 0 (shift 31)
    shifts: list = field(default_factory=lambda: [0] * 32)       # shifts[t]: steps of either kind that shifted by t, 1 <= t <= 31


@dataclass
class Wave:
    lanes: list
    iterations: int               # loop bodies the wave ran (even-fix and both-odd)


def _ctz32(w):
    return (w & -w).bit_length() - 1


def invert_wave(xs):
    """xs: up to 64 Montgomery-form values < p, one per lane of a wavefront"""
    n = len(xs)
    assert 1 <= n <= 64 and all(0 <= x < P for x in xs)
    u, v, r, s = [P] * n, list(xs), [0] * n, [1] * n
    active = [x != 0 for x in xs]
    out = [Lane() for _ in range(n)]
    iterations = 0
    for _ in range(LOOP_BOUND):
        if not any(active):
            break
        iterations += 1
        eu = [active[i] and not (u[i] & 1) for i in range(n)]
        ev = [active[i] and not (v[i] & 1) for i in range(n)]
        if any(eu[i] or ev[i] for i in range(n)):
            for i in range(n):
                wu = eu[i]
                w0 = (u[i] if wu else v[i]) & M32
                t = ((_ctz32(w0) if w0 else 31) if (eu[i] or ev[i]) else 0)
                tt = min(t, 31)
                if wu:
                    u[i] >>= tt
                    s[i] <<= tt
                    assert s[i] < 2 ** 256, "s << t carries out of 256 bits"
                else:
                    v[i] >>= tt
                    r[i] <<= tt
                    assert r[i] < 2 ** 256, "r << t carries out of 256 bits"
                out[i].k += tt
                if eu[i] or ev[i]:
                    out[i].even_fix += 1
                    out[i].even_fix_w0_zero += w0 == 0
                    out[i].shifts[tt] += 1
            continue
        for i in range(n):
            if not active[i]:          # the device computes these lanes too and keeps nothing
                continue
            d = u[i] - v[i]
            bw = d < 0
            d = abs(d)
            sm = r[i] + s[i]
            assert sm < 2 ** 256, "r + s carries out of 256 bits"
            nzd = d != 0
            gt = not bw and nzd
            d0 = d & M32
            t = ((_ctz32(d0) if d0 else 31) if nzd else 1)
            tt = min(t, 31)
            sh = (s[i] if gt else r[i]) << tt
            assert sh < 2 ** 256, ("s" if gt else "r") + " << t carries out of 256 bits"
            if gt:
                u[i], r[i], s[i] = d >> tt, sm, sh
            else:
                v[i], s[i], r[i] = d >> tt, sm, sh
            out[i].k += tt
            out[i].both_odd += 1
            out[i].both_odd_d0_zero += nzd and d0 == 0
            out[i].shifts[tt] += 1
            if not nzd:
                active[i] = False
    assert not any(active), "the loop's bound of %d iterations ended the inversion" % LOOP_BOUND
    for i in range(n):
        assert r[i] < 2 * P, "r >= 2p at the end"
        rr = r[i] - P if r[i] >= P else r[i]
        res = (0 - rr) % P
        if xs[i]:
            assert out[i].k < POW2_TAB_LEN, "k = %d is outside the table" % out[i].k
        out[i].result = res * pow(2, 768 - out[i].k, P) * RINV % P if xs[i] else 0
    return Wave(out, iterations)


def invert_all(xs):
    """xs laid out as the test hook launches them: 64 threads per block, inputs 64w .. 64w+63 share a wavefront"""
    return [invert_wave(xs[o:o + 64]) for o in range(0, len(xs), 64)]
