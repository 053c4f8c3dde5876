"""k_read_stats driven from count arrays built in numpy (needs a GPU): fk_read_stats_of_counts_device needs no result,
only the context's k, so every field of fk_read_stat is compared with np.sort over the valid windows of each read.

views_util.stat_batch: window counts on both sides of the 64-lane and the 256-register edges; no valid flags, all
ones, random halves, none, only below / only above window 256; values all equal (the mn == mx shortcut), two values
differing in bit 0, 1, 15, 16, 30 or 31 in ratios that put the median on either side, uniform 32-bit values, ascending,
descending, 1000 times 2^32 - 1 (a 42-bit sum), one outlier at either end.  About 2000 reads a batch, shuffled, so
each of a workgroup's four waves meets every shape; k = 1 (windows = length) and k = 31."""
import numpy as np
import pytest

import fastkmer_amd as fk
import views_util as vu

pytestmark = pytest.mark.gpu

MAX = fk.MAX_COUNT


def device_stats(kc, counts, valid, offsets, lo, hi):
    import torch
    n = len(offsets) - 1
    d_c = torch.from_numpy(counts.view(np.int32)).cuda() if len(counts) else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_v = None if valid is None else (torch.from_numpy(valid).cuda() if len(valid) else torch.zeros(1, dtype=torch.uint8, device="cuda"))
    d_o = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_s = torch.full((max(n, 1), 32), 0x55, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kc.read_stats_of_counts_ptr(d_c.data_ptr(), 0 if d_v is None else d_v.data_ptr(), d_o.data_ptr(), n, d_s.data_ptr(),
                                min_count=lo, max_count=hi)
    torch.cuda.synchronize()
    return d_s.cpu().numpy().reshape(-1).view(fk.READ_STAT_DTYPE)[:n]


def check(kc, counts, valid, offsets, lo, hi):
    got = device_stats(kc, counts, valid, offsets, lo, hi)
    want = vu.expected_select(counts, valid, offsets, kc.k, lo, hi)
    for f in fk.READ_STAT_DTYPE.names:
        bad = np.nonzero(got[f] != want[f])[0]
        lens = np.diff(offsets.astype(np.int64))
        assert len(bad) == 0, (f"{f} ({lo}, {hi}, valid {'given' if valid is not None else 'null'}) differs for reads "
                               f"{bad[:6]} of {lens[bad[:6]]} positions: {got[f][bad[:6]]} != {want[f][bad[:6]]}")
    return want


@pytest.mark.parametrize("k", [1, 31])
def test_read_stats_of_chosen_counts(k):
    counts, valid, offsets = vu.stat_batch(k, seed=k)
    with fk.KmerCounter(k, min(k, 7), 3, 64) as kc:  # nothing counted: the call reads only the context's k
        want = check(kc, counts, valid, offsets, 1, MAX)
        assert want["sum"].dtype == np.uint64 and int(want["sum"].max()) == 1000 * MAX > 2 ** 41
        assert ((want["min"] < want["median"]) & (want["median"] < want["max"])).any()
        assert (want["median"] >= 2 ** 31).any() and (want["windows"] == 0).any() and (want["windows"] == 1000).any()
        check(kc, counts, None, offsets, 1, MAX)
        for v in (valid, None):
            for lo, hi in ((2 ** 31, MAX), (7, 7), (MAX, MAX), (1000, 0x2A54)):
                w = check(kc, counts, v, offsets, lo, hi)
                assert (w["hits"] > 0).any() and (w["hits"] < w["windows"]).any()
        # batches that fill no workgroup, one, and one read more
        for n in (1, 3, 4, 5):
            for first in (0, 11):
                o = offsets[first:first + n + 1] - offsets[first]
                a, b = int(offsets[first]), int(offsets[first + n])
                check(kc, counts[a:b], valid[a:b], o, 2, MAX)
                check(kc, counts[a:b], None, o, 2, MAX)
