"""TEST SUPPORT: the inputs and the checks of the device field arithmetic's edge tests (fr_dev.hpp), shared by the CPU tests
(tests/test_fr_edges_cpu.py: the Python model of the inversion and the host build of the kernels) and the GPU tests
(tests/test_fr_edges_gpu.py: the device forms that exist only under __HIP_DEVICE_COMPILE__).

The inversion's inputs are MONTGOMERY-domain targets X: the values fr_inv_kaliski_inl itself sees.  pob_debug_fr_inv takes canonical
values and converts them, so it is fed c = X * R^-1 mod p and must return pow(c, p - 2, p).  The ORDER of the inputs is part of the
definition: the hook launches 64 threads per block, so inputs 64w .. 64w+63 share a wavefront, and a wavefront goes through the loop in
lock-step (an even-fix step of one lane is a step of every lane)."""
import ctypes
import random

from tests.fr_inv_model import P, R, RINV, invert_all

WAVE = 64


# ---------------------------------------------------------------------------------------------------------- inversion inputs
def _whole_waves(xs):
    """a family on a wave boundary: padded with idle lanes (0) up to the next one"""
    return xs + [0] * (-len(xs) % WAVE)


def _mixed_wave():
    """the shape of the emitter's call: idle lanes beside busy ones, unlike values side by side"""
    rng = random.Random(2311)
    xs = [0, 1, 2, P - 1]
    xs += [2 ** (31 * j) for j in range(1, 9)]
    xs += [P - 2 ** (32 * j) for j in range(1, 8)]
    xs += [3 * 2 ** (64 + j) for j in range(10)]
    xs += [rng.randrange(P) for _ in range(35)]
    assert len(xs) == WAVE
    return xs


def _small_families():
    xs = [P - 2 ** 32 * m for m in (1, 3, 5, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 100 + 7)]
    xs += [P - 2 ** 64 * m for m in (1, 3, 2 ** 64 + 1, 2 ** 150 + 9)]
    xs += [P - 2 ** 96 * m for m in (1, 5)]
    xs += [2 ** 32 * m for m in (3, 5, 2 ** 64 + 1)] + [7 * 2 ** 64, 3 * 2 ** 128, 3 * 2 ** 224]
    # the hand values of test_device_field_inversions, as targets and as the Montgomery forms that test's canonical inputs turn into
    hand = [4097, 65_535, P - 4097, 2 ** 253 % P]
    xs += hand + [h * R % P for h in hand]
    return xs


def inv_families():
    """[(name, Montgomery targets)], every family a whole number of waves"""
    rng = random.Random(2312)
    fams = [("2^j", _whole_waves([2 ** j for j in range(254)])),
            ("p-2^j", _whole_waves([P - 2 ** j for j in range(254)])),
            ("small", _whole_waves(_small_families())),
            ("p-2^(32+3j)", [P - 2 ** (32 + 3 * j) for j in range(64)]),
            ("mixed", _mixed_wave()),
            ("random", [rng.randrange(P) for _ in range(2 * WAVE)])]
    for name, xs in fams:
        assert len(xs) % WAVE == 0 and all(0 <= x < P for x in xs), name
    return fams


def inv_targets():
    """the whole set in launch order"""
    return [x for _, xs in inv_families() for x in xs]


def inv_partial_calls():
    """separate launches whose last wavefront is partial (the kernel returns early for t >= n, the loop's __any then runs on the rest): n = 1, 37, 64 + 37"""
    mixed = _mixed_wave()
    calls = [[P - 2 ** 64],
             mixed[:20] + [P - 2 ** j for j in range(32, 49)],
             mixed + [P - 2 ** (32 + 5 * i) for i in range(37)]]
    assert [len(c) for c in calls] == [1, 37, 101]
    return calls


def to_canonical(X):
    return X * RINV % P


def _pack(xs):
    return b"".join(x.to_bytes(32, "little") for x in xs)


def _unpack(raw):
    return [int.from_bytes(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]


def check_fr_inv(lib, targets, fermat=True):
    """pob_debug_fr_inv on the canonical forms of the Montgomery targets: the Kaliski output (and the Fermat ladder's) against pow"""
    cs = [to_canonical(X) for X in targets]
    buf = _pack(cs)
    a, b = ctypes.create_string_buffer(len(buf)), ctypes.create_string_buffer(len(buf))
    assert lib.pob_debug_fr_inv(0, buf, len(cs), a, b) == 0
    ka, fe = _unpack(a.raw), _unpack(b.raw)
    bad = [(i, hex(targets[i])) for i, c in enumerate(cs) if ka[i] != pow(c, P - 2, P)]
    assert not bad, ("Kaliski inversion", len(bad), bad[:4])
    if fermat:
        bad = [(i, hex(targets[i])) for i, c in enumerate(cs) if fe[i] != pow(c, P - 2, P)]
        assert not bad, ("Fermat inversion", len(bad), bad[:4])


# ---------------------------------------------------------------------------------------------------------- the binary operations
# op codes of pob_debug_fr_ops (include/pob_hip.h POB_FR_OP_*)
OP_MUL, OP_MUL_INL, OP_ADD, OP_SUB, OP_NEG, OP_TO_MONT, OP_FROM_MONT, OP_FROM_I64 = range(8)
NPRIME = -pow(P, -1, 2 ** 256) % 2 ** 256


def fr_sqr_values():
    """the value list of check_fr_sqr (tests/test_poseidon_lanes_cpu.py, which builds it inside the check; the same construction here, and
    tests/test_fr_edges_cpu.py holds the two equal): zero, one, the limb boundaries, values next to p and to 2^253, values that make the final conditional
    subtraction of the square run, and random values"""
    rng = random.Random(5)
    xs = [0, 1, 2, 3, P - 1, P - 2, P - 3, (P - 1) // 2, (P + 1) // 2, 2 ** 253, 2 ** 253 - 1, 2 ** 253 % P, 2 ** 128, 2 ** 128 - 1, 2 ** 127 + 1]
    xs += [2 ** (32 * k) - 1 for k in range(1, 8)] + [2 ** (32 * k) for k in range(1, 8)] + [P - 2 ** (32 * k) for k in range(1, 8)]
    xs += [2 ** 256 % P, 2 ** 512 % P]
    # values whose product-scanning result lands in [p, 2p) before the final subtraction (most random values do not)
    over = [x for x in (rng.randrange(P) for _ in range(4000)) if (x * x + (x * x * NPRIME % 2 ** 256) * P) >> 256 >= P]
    assert len(over) >= 16
    xs += over[:64]
    xs += [rng.randrange(P) for _ in range(300)] + [rng.randrange(2 ** 32) for _ in range(20)] + [P - 1 - rng.randrange(2 ** 64) for _ in range(20)]
    return xs


def unreduced_product(a, b):
    """what product scanning holds before its final conditional subtraction: (a*b + m*p) / 2^256 < 2p"""
    return (a * b + (a * b * NPRIME % 2 ** 256) * P) >> 256


def mul_pairs():
    """operand pairs (a, b), all < p, for fr_mul / fr_mul_inl (and reused for fr_add / fr_sub)"""
    rng = random.Random(2313)
    vals = fr_sqr_values()
    # (1) check_fr_sqr's values crossed pairwise: its 38 hand values all against each other both ways would be 1 406 pairs -- a seeded subset, a != b
    hand = vals[:38]
    cross = [(a, b) for a in hand for b in hand if a != b]
    pairs = rng.sample(cross, 300)
    while len(pairs) < 480:
        a, b = rng.choice(vals), rng.choice(vals)
        if a != b:
            pairs.append((a, b))
    assert len(pairs) >= 400 and all(a != b for a, b in pairs)
    # (2) every limb 0xFFFFFFFF except the top one: all 16 column sums of a*b at their largest (top limb of p: 0x30644e72, the limb below it < 0xFFFFFFFF)
    tops = [0x30644e71, 0x30644e70, 0x2fffffff, 0x20000000, 0x00000001, 0x00000000]
    ones = [(t << 224) | (2 ** 224 - 1) for t in tops]
    assert all(x < P for x in ones)
    pairs += [(a, b) for a in ones for b in ones]
    # (3) pairs whose unreduced product-scanning result lies in [p, 2p): the final subtraction runs (selected as check_fr_sqr selects `over`)
    over = [ab for ab in ((rng.randrange(P), rng.randrange(P)) for _ in range(4000)) if unreduced_product(*ab) >= P]
    assert len(over) >= 16
    pairs += over[:64]
    # (4) random pairs
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(2000)]
    return pairs


def add_sub_pairs():
    rng = random.Random(2314)
    some = [1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 224 - 1, (P - 1) // 2, (P + 1) // 2, P - 2, P - 1] + [rng.randrange(2, P - 1) for _ in range(8)]
    pairs = []
    for a in some:                                     # a + b == p, p - 1, p + 1 (b < p: a >= 1 / a >= 0 / a >= 2)
        pairs += [(a, P - a), (a, P - 1 - a)]
        if a >= 2:
            pairs.append((a, P + 1 - a))
    pairs += [(0, P - 1), (P - 1, 0), (0, 0), (P - 1, P - 1)]
    pairs += [(0, 1), (P - 1, 0), (0, P - 1), (1, 0), (1, 2), (2 ** 32, 1), (2 ** 224, 1), (0, 2 ** 224)] + [(a, a) for a in some]      # 0 - 1, a - a, (p-1) - 0, 0 - (p-1), borrows through limbs
    assert all(0 <= a < P and 0 <= b < P for a, b in pairs)
    return pairs + mul_pairs()


def unary_values():
    return [0, 1, P - 1] + fr_sqr_values() + [a for a, _ in mul_pairs()[-500:]]


I64_VALUES = [0, 1, -1, 4096, -4096, 4097, -4097, 2 ** 63 - 1, -(2 ** 63 - 1)]          # (INT64_MIN: -k is undefined for it and no caller passes it)


def _run_op(lib, op, a, b=None):
    n = len(a)
    out = ctypes.create_string_buffer(32 * n)
    assert lib.pob_debug_fr_ops(0, op, _pack(a), _pack(b) if b is not None else None, n, out) == 0, op
    return _unpack(out.raw)


def _cmp(name, got, want, ops):
    bad = [(i, [hex(x) for x in ops[i]], hex(got[i]), hex(want[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (name, len(bad), bad[:3])


def check_fr_ops(lib):
    """pob_debug_fr_ops, raw limbs in and out, against Python's big integers: a*b*2^-256, a +- b, -a, a*2^(+-256), k*2^256, all mod p"""
    mp = mul_pairs()
    a, b = [x for x, _ in mp], [y for _, y in mp]
    want = [x * y * RINV % P for x, y in mp]
    assert sum(unreduced_product(x, y) >= P for x, y in mp) >= 16
    _cmp("fr_mul", _run_op(lib, OP_MUL, a, b), want, mp)
    _cmp("fr_mul_inl", _run_op(lib, OP_MUL_INL, a, b), want, mp)
    _cmp("fr_mul (operands swapped)", _run_op(lib, OP_MUL, b, a), want, mp)
    ap = add_sub_pairs()
    a, b = [x for x, _ in ap], [y for _, y in ap]
    _cmp("fr_add", _run_op(lib, OP_ADD, a, b), [(x + y) % P for x, y in ap], ap)
    _cmp("fr_sub", _run_op(lib, OP_SUB, a, b), [(x - y) % P for x, y in ap], ap)
    un = unary_values()
    u1 = [(x,) for x in un]
    got = _run_op(lib, OP_NEG, un)
    assert got[0] == 0, "neg(0) != 0"
    _cmp("fr_neg", got, [-x % P for x in un], u1)
    _cmp("fr_to_mont", _run_op(lib, OP_TO_MONT, un), [x * R % P for x in un], u1)
    _cmp("fr_from_mont", _run_op(lib, OP_FROM_MONT, un), [x * RINV % P for x in un], u1)
    ks = [k % 2 ** 64 for k in I64_VALUES]             # the low 8 bytes of a, read as a signed value
    _cmp("fr_from_i64", _run_op(lib, OP_FROM_I64, ks), [k * R % P for k in I64_VALUES], [(k,) for k in I64_VALUES])
    # argument checks of the hook itself: an unknown op, a binary op without b
    out = ctypes.create_string_buffer(32)
    assert lib.pob_debug_fr_ops(0, 8, _pack([1]), _pack([1]), 1, out) != 0
    assert lib.pob_debug_fr_ops(0, OP_ADD, _pack([1]), None, 1, out) != 0
