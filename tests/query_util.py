"""numpy helpers shared by test_query.py and test_gpu_query.py: 2-bit k-mer keys as (hi, lo) uint64
arrays (hi = 0 for k <= 32), their reverse complements, and expected lookup answers from the oracle's
per-bin arrays -- no Python dicts of k-mers."""
import ctypes

import numpy as np

import fastkmer_amd as fk

U64 = np.uint64
CONFIGS = [(28, 10, 2048), (21, 7, 64), (32, 11, 256), (55, 12, 8192), (63, 15, 512)]


def _rev_pairs(x):
    """The 32 two-bit groups of every uint64 in reverse order."""
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap()


def revcomp(hi, lo, k):
    """Reverse complement of 2k-bit keys: complement every base, reverse their order."""
    rh, rl = _rev_pairs(~lo), _rev_pairs(~hi)  # the 128-bit reversal: reversed lo is the high word
    s = 128 - 2 * k
    if s >= 64:
        return np.zeros_like(hi), rh >> U64(s - 64) if s > 64 else rh.copy()
    if s == 0:
        return rh, rl
    return rh >> U64(s), (rl >> U64(s)) | (rh << U64(64 - s))


def canonical(hi, lo, k):
    rh, rl = revcomp(hi, lo, k)
    less = (rh < hi) | ((rh == hi) & (rl < lo))
    return np.where(less, rh, hi), np.where(less, rl, lo)


def is_kmer(hi, lo, k):
    """No bit above bit 2k - 1."""
    if k >= 64:
        return np.ones(len(lo), dtype=bool)
    if k > 32:
        return (hi >> U64(2 * k - 64)) == 0
    return (hi == 0) & ((lo >> U64(2 * k)) == 0 if k < 32 else True)


def pack(hi, lo, k):
    """(hi, lo) -> a flat uint64 array in fk_get_bin's layout."""
    if k <= 32:
        return np.ascontiguousarray(lo, dtype=U64)
    return np.ascontiguousarray(np.stack([hi, lo], axis=1).reshape(-1), dtype=U64)


def add(hi, lo, d):
    """keys + d (d = 1 or -1) as 128-bit integers, wrapping."""
    with np.errstate(over="ignore"):
        if d == 1:
            nl = lo + U64(1)
            return hi + (nl == 0).astype(U64), nl
        nl = lo - U64(1)
        return hi - (lo == 0).astype(U64), nl


class OracleTable:
    """Every distinct canonical k-mer of an oracle.OracleResult as arrays: hi, lo, count, bin (bins in
    order, keys ascending inside a bin), and first / last = the index range of every non-empty bin."""

    def __init__(self, res, nbins, bins=None):
        his, los, cnts, bns, self.first, self.last = [], [], [], [], [], []
        at = 0
        for b in (range(nbins) if bins is None else bins):
            hi, lo, cnt = res.bin_arrays(b)
            if len(lo) == 0:
                continue
            his.append(hi), los.append(lo), cnts.append(cnt), bns.append(np.full(len(lo), b, dtype=np.int32))
            self.first.append(at)
            at += len(lo)
            self.last.append(at - 1)
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
        self.hi, self.lo = cat(his, U64), cat(los, U64)
        self.count, self.bin = cat(cnts, np.uint32), cat(bns, np.int32)

    def __len__(self):
        return len(self.lo)

    def find(self, qhi, qlo, k):
        """The index in the table of every query key (either strand), -1 for a k-mer it does not hold."""
        chi, clo = canonical(qhi, qlo, k)
        n = len(self)
        hi, lo = np.concatenate([self.hi, chi]), np.concatenate([self.lo, clo])
        order = np.lexsort((lo, hi))
        sh, sl = hi[order], lo[order]
        new = np.ones(len(order), dtype=np.int64)
        new[1:] = (sh[1:] != sh[:-1]) | (sl[1:] != sl[:-1])
        gid = np.empty(len(order), dtype=np.int64)
        gid[order] = np.cumsum(new) - 1
        at = np.full(int(gid.max()) + 1 if len(gid) else 0, -1, dtype=np.int64)
        at[gid[:n]] = np.arange(n)
        return at[gid[n:]]

    def expected(self, qhi, qlo, k):
        """The oracle's count of every query key (either strand): 0 for a k-mer it does not hold."""
        at = self.find(qhi, qlo, k)
        table = np.concatenate([self.count, np.zeros(1, dtype=np.uint32)])  # index -1: absent
        return table[at]


def kmer_bins(keys, k, m, B):
    """fk_kmer_bin of every key of a flat array in fk_get_bin's layout (one C call per key)."""
    L = fk.lib()
    keys = np.ascontiguousarray(keys, dtype=U64)
    kw = 2 if k > 32 else 1
    n = keys.size // kw
    cfg = fk.make_config(k, m, 1, B)
    out = np.full(n, -2, dtype=np.int32)
    f, cref = L.fk_kmer_bin, ctypes.byref(cfg)
    if n == 0:
        return out
    ka, oa = keys.ctypes.data, out.ctypes.data
    for i in range(n):
        if f(cref, ka + 8 * kw * i, oa + 4 * i) != 0:
            raise fk.FastKmerError(-1, L.fk_last_error().decode())
    return out
