"""Host statement of the dropout mask of msr3d_amd/csrc/dropout_rng.h, in numpy with wrapping unsigned
32 / 64-bit arithmetic.  The kernels regenerate the mask from (seed word, call-site salt, element index)
and store none, so this module is the only place outside them that says WHICH elements are dropped;
tests/test_dropout_sites_gpu.py ties it to every kernel that draws a mask.

Index convention (every site): the element's flat offset in its buffer, truncated to 32 bits -- rows of
D columns use row * D + col, the feed-forward sites row * FF + col, `row` counted over all B * L token
rows (never per scene or per 64-row tile).
"""
import numpy as np

MASK64 = (1 << 64) - 1
LCG_MUL, LCG_ADD = 6364136223846793005, 1442695040888963407


def u64(seed):
    """The seed word as the kernels read it: the int64 tensor's value as 64 unsigned bits."""
    return int(seed) & MASK64


def bump(seed):
    """msr3d_bump_seed: seed * 6364136223846793005 + 1442695040888963407 mod 2^64."""
    return (u64(seed) * LCG_MUL + LCG_ADD) & MASK64


def drop_mix32(h):
    """murmur3 finaliser on uint32 arrays (wrapping)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def drop_thresh(p):
    """(unsigned)(p * 65536.0 + 0.5) with p an fp32 value; 0 for p <= 0."""
    p32 = np.float32(p)
    return int(np.float64(p32) * 65536.0 + 0.5) if p32 > 0 else 0


def scale(p):
    """The inverted-dropout factor as the kernels form it, in fp32: 1.0f / (1.0f - p)."""
    p32 = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p32) if p32 > 0 else np.float32(1.0)


def _site_constant(seed, salt):
    s = u64(seed)
    lo, hi = s & 0xFFFFFFFF, s >> 32
    c = drop_mix32(np.uint32(lo ^ ((int(salt) * 0x7FEB352D) & 0xFFFFFFFF)))
    return np.uint32((int(c) + hi) & 0xFFFFFFFF)


def bits16(seed, salt, idx, swap_halves=False, per_element=False):
    """The 16 bits element `idx` compares with the threshold: one hash per PAIR (idx >> 1), its low half
    for even idx, its high half for odd idx.  swap_halves / per_element are deliberately WRONG variants
    (halves exchanged; idx hashed instead of idx >> 1) for tests that show the comparison can fail."""
    idx = np.asarray(idx, dtype=np.uint64).astype(np.uint32)          # 32-bit truncation
    c = _site_constant(seed, salt)
    with np.errstate(over="ignore"):
        key = idx if per_element else idx >> np.uint32(1)
        h = drop_mix32(key * np.uint32(0x9E3779B1) + c)
    odd = (idx & np.uint32(1)).astype(bool) ^ bool(swap_halves)
    return np.where(odd, h >> np.uint32(16), h & np.uint32(0xFFFF))


def keep_elem(seed, salt, idx, thresh, **variant):
    """True where element `idx` is KEPT: bits >= thresh, P(keep) = 1 - thresh / 2^16."""
    return bits16(seed, salt, idx, **variant) >= np.uint32(thresh)


def keep_mask(seed, salt, rows, ld, cols, p, row0=0, **variant):
    """(rows, cols) bool: element (r, c) uses index (row0 + r) * ld + c, truncated to 32 bits."""
    r = np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(row0)
    idx = r * np.uint64(ld) + np.arange(cols, dtype=np.uint64)[None, :]
    return keep_elem(seed, salt, idx, drop_thresh(p), **variant)
