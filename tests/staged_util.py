"""Synthetic staged pieces for KmerCounter.debug_count_pieces, and the plain reference of their count.

A piece is a triple (bins, kmers, weights) of equal length: the bin of every entry, its k-mer
(uint64 for k <= 32, (hi, lo) rows for k > 32) and its weight (1 for an unweighted entry).  layout()
turns pieces into the key arrays and cell counts the count's staged format wants; reference() is
the count they must give: per bin, np.unique of the k-mers with the weights summed in int64.
Nothing here needs a GPU (bins_of calls the library's host-only fk_kmer_bin).
"""
import ctypes

import numpy as np

import fastkmer_amd as fk

U64 = np.uint64


def kw_of(k):
    return 1 if k <= 32 else 2


def as_kmers(kmers, k):
    a = np.ascontiguousarray(kmers, dtype=U64)
    return a.reshape(-1) if k <= 32 else a.reshape(-1, 2)


def cell_of(kmers, k, F):
    """The top F bits of the 2k-bit k-mers."""
    km = as_kmers(kmers, k)
    sh = 2 * k - F
    if k <= 32:
        return (km >> U64(sh)).astype(np.int64)
    hi, lo = km[:, 0], km[:, 1]
    if sh >= 64:
        return (hi >> U64(sh - 64)).astype(np.int64)
    return ((hi << U64(64 - sh)) | (lo >> U64(sh))).astype(np.int64)


def bins_of(kmers, k, m, B):
    """The bin of every k-mer under (k, m, B), by the library's host-side fk_kmer_bin."""
    km = as_kmers(kmers, k)
    out = np.zeros(len(km), dtype=np.int64)
    if fk.clamped_bins(m, B) == 1:
        return out
    cfg = fk.make_config(k, m, 1, B)
    b = ctypes.c_int32(-1)
    fn = fk.lib().fk_kmer_bin
    for i in range(len(km)):
        key = np.ascontiguousarray(km[i]).reshape(-1)
        fk._check(fn(ctypes.byref(cfg), key.ctypes.data, ctypes.byref(b)))
        out[i] = b.value
    return out


def distinct_kmers(rng, k, F, cell, n, m=None, B=1, want_bin=0, low_bits=None):
    """n distinct k-mers of cell `cell` (of F cell bits) that lie in bin want_bin of B, ascending.
    low_bits: only that many low bits differ between them."""
    sh = 2 * k - F
    free = sh if low_bits is None else min(low_bits, sh)
    if free < 63 and (1 << free) < n:
        raise ValueError(f"cell holds {1 << free} k-mers, {n} wanted")
    got = np.zeros(0, dtype=U64) if k <= 32 else np.zeros((0, 2), dtype=U64)
    while len(got) < n:
        want = (n - len(got)) * (2 * B if B > 1 else 1) + 16
        if k <= 32:
            lows = rng.integers(0, 1 << free, want, dtype=U64) if free else np.zeros(want, dtype=U64)
            cand = (U64(cell) << U64(sh)) | lows if sh else np.full(want, cell, dtype=U64)
            cand = cand[cand != U64(0xFFFFFFFFFFFFFFFF)]  # the empty-slot marker (all T at k = 32)
        else:
            lo = rng.integers(0, 1 << min(free, 64), want, dtype=U64, endpoint=False) if free < 64 else \
                rng.integers(0, 0xFFFFFFFFFFFFFFFF, want, dtype=U64, endpoint=True)
            hi = np.zeros(want, dtype=U64)
            if free > 64:
                hi = rng.integers(0, 1 << (free - 64), want, dtype=U64)
            if sh >= 64:
                hi |= U64(cell) << U64(sh - 64)
            else:
                hi |= U64(cell >> (64 - sh))
                lo = (lo & U64((1 << sh) - 1)) | (U64(cell & ((1 << (64 - sh)) - 1)) << U64(sh))
            cand = np.stack([hi, lo], axis=1)
        if B > 1:
            cand = cand[bins_of(cand, k, m, B) == want_bin]
        got = np.unique(np.concatenate([got, cand]), axis=0) if k > 32 else np.unique(np.concatenate([got, cand]))
    pick = np.sort(rng.choice(len(got), n, replace=False))
    return got[pick]


def cell_entries(rng, kmers, n, weighted=False, heavy=False):
    """n entries over the given distinct k-mers (each at least once; heavy: the first takes most of
    the rest), weights 1..15 with both ends present where there is room (else all 1)."""
    d = len(kmers)
    assert 1 <= d <= n
    extra = n - d
    if heavy and extra:
        idx = np.concatenate([np.arange(d), np.zeros(extra - extra // 4, dtype=np.int64), rng.integers(0, d, extra // 4)])
    else:
        idx = np.concatenate([np.arange(d), rng.integers(0, d, extra)])
    w = np.ones(n, dtype=np.int64)
    if weighted:
        w = rng.integers(1, 16, n).astype(np.int64)
        w[0] = 15
        if n > 1:
            w[-1] = 1
    return kmers[idx], w


def piece(bins, kmers, weights, k):
    km = as_kmers(kmers, k)
    b = np.broadcast_to(np.asarray(bins, dtype=np.int64), (len(km),)).copy()
    w = np.broadcast_to(np.asarray(weights, dtype=np.int64), (len(km),)).copy()
    return b, km, w


def concat_pieces(parts, k):
    """One piece out of several (bins, kmers, weights) triples."""
    if not parts:
        return piece(np.zeros(0, dtype=np.int64), np.zeros(0 if k <= 32 else (0, 2), dtype=U64), np.zeros(0, dtype=np.int64), k)
    return (np.concatenate([p[0] for p in parts]), np.concatenate([as_kmers(p[1], k) for p in parts]),
            np.concatenate([p[2] for p in parts]))


def spread(rng, whole, n_pieces, k, how="random"):
    """One piece's entries dealt over n_pieces: "random", "last" (all in the last piece), or
    "not_first" (piece 0 holds none)."""
    b, km, w = whole
    if how == "last":
        at = np.full(len(b), n_pieces - 1)
    elif how == "not_first" and n_pieces > 1:
        at = rng.integers(1, n_pieces, len(b))
    else:
        at = rng.integers(0, n_pieces, len(b))
    return [(b[at == p], km[at == p], w[at == p]) for p in range(n_pieces)]


def one_cell(rng, k, F, cell, n, d, weighted=False, heavy=False, m=None, B=1, bn=0, low_bits=None):
    """One cell's n entries over d distinct k-mers, as a piece."""
    km = distinct_kmers(rng, k, F, cell, d, m, B, bn, low_bits)
    e, w = cell_entries(rng, km, n, weighted, heavy)
    return piece(bn, e, w, k)


MODES = ("random", "last", "not_first")


def deal(rng, cells, n_pieces, k, modes=MODES):
    """The cells' entries dealt over n_pieces, cell i by modes[i % len(modes)] (see spread): with
    several pieces some cells lie in the last piece only and some miss the first."""
    per = [spread(rng, c, n_pieces, k, modes[i % len(modes)]) for i, c in enumerate(cells)]
    return [concat_pieces([pc[p] for pc in per], k) for p in range(n_pieces)]


def layout(pieces, k, F, B, rng, weighted=False, order="random"):
    """pieces -> (keys per piece, cell counts per piece) in the staged format: every piece's keys by
    (bin, cell), in random order inside a cell (order "asc" / "desc": by k-mer); a weighted key holds
    weight - 1 in bits [2k, 2k + 4)."""
    keys, counts = [], []
    for b, km, w in pieces:
        km = as_kmers(km, k)
        w = np.asarray(w, dtype=np.int64)
        if len(w) and (w.min() < 1 or w.max() > (15 if weighted else 1)):
            raise ValueError("weights: 1..15 in a weighted layout, else 1")
        if weighted and 2 * k > 60:
            raise ValueError("no weight field above k = 30")
        g = (np.asarray(b, dtype=np.int64) << F) | cell_of(km, k, F)
        if order == "random":
            perm = rng.permutation(len(g))
        else:
            perm = np.argsort(km, kind="stable") if k <= 32 else np.lexsort((km[:, 1], km[:, 0]))
            if order == "desc":
                perm = perm[::-1]
        at = perm[np.argsort(g[perm], kind="stable")]
        out = km[at].copy()
        if weighted:
            out |= (w[at].astype(U64) - U64(1)) << U64(2 * k)
        keys.append(out.reshape(-1))
        counts.append(np.bincount(g, minlength=B << F).astype(U64))
    return keys, counts


def reference(pieces, k, B):
    """{bin: (distinct k-mers ascending, int64 counts = summed weights)} over all pieces."""
    b, km, w = concat_pieces(list(pieces), k)
    out = {}
    for bn in range(B):
        sel = b == bn
        if k <= 32:
            u, inv = np.unique(km[sel], return_inverse=True)
        else:
            u, inv = np.unique(km[sel], axis=0, return_inverse=True)
        c = np.zeros(len(u), dtype=np.int64)
        np.add.at(c, inv.reshape(-1), w[sel].astype(np.int64))
        out[bn] = (u, c)
    return out


def split_weighted(keys, k):
    """Weighted staged keys (k <= 30) -> (k-mers, weights)."""
    keys = np.asarray(keys, dtype=U64)
    return keys & U64((1 << (2 * k)) - 1), (keys >> U64(2 * k)).astype(np.int64) + 1


def assert_counted(kc, ref, ordered=True):
    """Every bin of the counter equals the reference (as sets when not ordered), and the totals."""
    B = kc.num_bins
    sizes = kc.bin_sizes()
    total = distinct = 0
    for bn in range(B):
        ek, ec = ref[bn]
        total += int(ec.sum())
        distinct += len(ek)
        assert int(sizes[bn]) == len(ek), f"bin {bn}: {int(sizes[bn])} k-mers, expected {len(ek)}"
        gk, gc = kc.get_bin(bn)
        gk = as_kmers(gk, kc.k)
        gc = gc.astype(np.int64)
        if not ordered and len(gk):
            o = np.lexsort((gk[:, 1], gk[:, 0])) if kc.k > 32 else np.argsort(gk, kind="stable")
            gk, gc = gk[o], gc[o]
        assert np.array_equal(gk, ek), f"bin {bn}: keys differ"
        bad = np.nonzero(gc != ec)[0]
        assert len(bad) == 0, f"bin {bn}: {len(bad)} counts differ, first at {bad[:1]}: {gc[bad[:1]]} != {ec[bad[:1]]}"
    st = kc.stats()
    assert st["kmers"] == total and st["distinct"] == distinct, (st["kmers"], total, st["distinct"], distinct)
