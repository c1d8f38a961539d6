"""TEST INFRASTRUCTURE: the packed window format (version 1) in numpy -- the format's independent statement, written from its specification (INTEGRATION.md
"Packed windows"), not from the library's C++.  encode() is what the device pass must produce byte for byte, decode() what pob_unpack_window must return.

One packed window describes n consecutive payload positions.  All integers little-endian, every section starts on a 32-byte boundary, padding bytes are zero:
  1. header, 32 bytes: u32 magic 'POBP', u32 version = 1, u64 first_wire, u32 n_wires, u32 n_small, u32 n_wide, u32 0
  2. tag planes, ceil(n / 64) pairs of u64 {lo, hi}: bit i % 64 of pair i // 64 gives wire i's tag hi << 1 | lo.  0: the value 0; 1: the value 1;
     2 ("small"): 2 <= value < 2^32; 3 ("wide"): anything else.  Bits beyond n are zero
  3. chunk index, ceil(n / 4096) pairs of u32 {small_before, wide_before}
  4. small values, n_small x u32, wire order
  5. wide values, n_wide x 32 bytes canonical LE, wire order
"""
import numpy as np

MAGIC = b"POBP"
VERSION = 1
CHUNK = 4096


def _pad32(b: int) -> int:
    return (b + 31) // 32 * 32


def section_offsets(n: int, n_small: int, n_wide: int):
    """byte offsets of (tag planes, chunk index, small values, wide values, end of the window)"""
    planes = 32
    index = planes + _pad32(16 * ((n + 63) // 64))
    small = index + _pad32(8 * ((n + CHUNK - 1) // CHUNK))
    wide = small + _pad32(4 * n_small)
    return planes, index, small, wide, wide + 32 * n_wide


def packed_size(n: int, n_small: int, n_wide: int) -> int:
    return section_offsets(n, n_small, n_wide)[4]


def tags_of(vals) -> np.ndarray:
    v = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1, 32)
    low = v[:, :4].copy().view("<u4").ravel()
    narrow = ~v[:, 4:].any(axis=1)
    return np.where(narrow, np.minimum(low, 2), 3).astype(np.uint8)


def counts_of(vals):
    """(n, n_small, n_wide) of canonical values"""
    t = tags_of(vals)
    return int(t.size), int((t == 2).sum()), int((t == 3).sum())


def encode(vals, first_wire: int = 0) -> np.ndarray:
    """canonical values (uint8, 32 bytes per wire) -> the packed window as a uint8 array"""
    v = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1, 32)
    n = v.shape[0]
    tag = tags_of(v)
    small, wide = tag == 2, tag == 3
    n_small, n_wide = int(small.sum()), int(wide.sum())
    o_planes, o_index, o_small, o_wide, total = section_offsets(n, n_small, n_wide)
    out = np.zeros(total, dtype=np.uint8)
    out[0:4] = np.frombuffer(MAGIC, dtype=np.uint8)
    out[4:8] = np.frombuffer(np.array([VERSION], dtype="<u4").tobytes(), dtype=np.uint8)
    out[8:16] = np.frombuffer(np.array([first_wire], dtype="<u8").tobytes(), dtype=np.uint8)
    out[16:28] = np.frombuffer(np.array([n, n_small, n_wide], dtype="<u4").tobytes(), dtype=np.uint8)
    nblk = (n + 63) // 64
    t = np.zeros(nblk * 64, dtype=np.uint8)
    t[:n] = tag
    planes = np.empty((nblk, 2, 8), dtype=np.uint8)
    planes[:, 0, :] = np.packbits((t & 1).reshape(nblk, 64), axis=1, bitorder="little")
    planes[:, 1, :] = np.packbits((t >> 1).reshape(nblk, 64), axis=1, bitorder="little")
    out[o_planes:o_planes + 16 * nblk] = planes.ravel()
    starts = np.arange(0, n, CHUNK)
    cs = np.concatenate([[0], np.cumsum(small)])[starts]
    cw = np.concatenate([[0], np.cumsum(wide)])[starts]
    idx = np.stack([cs, cw], axis=1).astype("<u4")
    out[o_index:o_index + idx.nbytes] = np.frombuffer(idx.tobytes(), dtype=np.uint8)
    out[o_small:o_small + 4 * n_small] = v[small, :4].ravel()
    out[o_wide:o_wide + 32 * n_wide] = v[wide].ravel()
    return out


def decode(buf) -> tuple:
    """a packed window -> (first_wire, canonical values as uint8 [32 * n]); asserts the consistency a reader must check"""
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    assert b[0:4].tobytes() == MAGIC
    version, = np.frombuffer(b[4:8].tobytes(), dtype="<u4")
    first_wire, = np.frombuffer(b[8:16].tobytes(), dtype="<u8")
    n, n_small, n_wide, zero = (int(x) for x in np.frombuffer(b[16:32].tobytes(), dtype="<u4"))
    assert version == VERSION and zero == 0
    o_planes, o_index, o_small, o_wide, total = section_offsets(n, n_small, n_wide)
    assert b.size == total
    nblk = (n + 63) // 64
    planes = b[o_planes:o_planes + 16 * nblk].reshape(nblk, 2, 8)
    lo = np.unpackbits(planes[:, 0, :], axis=1, bitorder="little").ravel()
    hi = np.unpackbits(planes[:, 1, :], axis=1, bitorder="little").ravel()
    assert not lo[n:].any() and not hi[n:].any()
    tag = (hi[:n] << 1 | lo[:n])
    small, wide = tag == 2, tag == 3
    assert int(small.sum()) == n_small and int(wide.sum()) == n_wide
    starts = np.arange(0, n, CHUNK)
    idx = np.frombuffer(b[o_index:o_index + 8 * starts.size].tobytes(), dtype="<u4").reshape(-1, 2)
    assert np.array_equal(idx[:, 0], np.concatenate([[0], np.cumsum(small)])[starts]) and np.array_equal(idx[:, 1], np.concatenate([[0], np.cumsum(wide)])[starts])
    v = np.zeros((n, 32), dtype=np.uint8)
    v[tag == 1, 0] = 1
    v[small, :4] = b[o_small:o_small + 4 * n_small].reshape(-1, 4)
    v[wide] = b[o_wide:o_wide + 32 * n_wide].reshape(-1, 32)
    return int(first_wire), v.ravel()
