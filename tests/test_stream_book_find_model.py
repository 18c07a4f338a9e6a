"""The model of the book by digest (tests/stream_book_find_model.py) against an O(n |B|) scan, and
the interface it is the yardstick of: libydc.so exports the two calls, the binding has the two
methods. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import stream_book_find_model as FM
from tests.conftest import ROOT
from yadcc_amd import binding, streaming

EDGE = (0, (1 << 64) - 1)


def random_book(n, alphabet, seed):
    """n entries whose keys are drawn from `alphabet` values (0 and all-ones among them)."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.array(EDGE, np.uint64)[:min(2, alphabet)],
                           rng.integers(1, 1 << 63, max(alphabet - 2, 0), dtype=np.uint64)])[:max(alphabet, 1)]
    return (rng.integers(0, 50, n).astype(np.uint32), rng.integers(1, 1 << 40, n, dtype=np.uint64),
            rng.integers(1, 1 << 62, n, dtype=np.uint64), pool[rng.integers(0, len(pool), n)] if n else pool[:0])


def scan(columns, key):
    """The last entry with `key` and how many there are, by looking at every entry."""
    pos = [p for p in range(len(columns[3])) if int(columns[3][p]) == key]
    return (pos[-1], len(pos)) if pos else (None, 0)


@pytest.mark.parametrize("n", [0, 1, 37, 300])
@pytest.mark.parametrize("alphabet", [1, 7, None])
def test_find_is_the_last_entry_and_the_count(n, alphabet):
    cols = random_book(n, alphabet or max(n, 1), seed=n + 3)
    absent = [3, 5, (1 << 64) - 2]
    keys = sorted(set(cols[3].tolist())) + absent + list(EDGE) + cols[3][:5].tolist()  # (queries repeat)
    got = FM.find(cols, np.array(keys, np.uint64))
    assert got.dtype.itemsize == 32 and len(got) == len(keys)
    for h, key in zip(got, keys):
        p, cnt = scan(cols, key)
        if p is None:
            assert tuple(h) == FM.MISS
        else:
            assert (int(h["pos"]), int(h["count"]), int(h["reserved"])) == (p, cnt, 0)
            assert (int(h["servant_idx"]), int(h["task_grant_id"]), int(h["servant_task_id"])) == (
                int(cols[0][p]), int(cols[1][p]), int(cols[2][p]))


@pytest.mark.parametrize("n", [0, 1, 37, 300])
@pytest.mark.parametrize("alphabet", [1, 7, None])
def test_distinct_is_the_map_after_the_pass_in_position_order(n, alphabet):
    cols = random_book(n, alphabet or max(n, 1), seed=n + 11)
    srv, gid, stid, dkey, cnt = FM.distinct(cols)
    m = {}
    for p in range(n):  # the reference's pass
        m[int(cols[3][p])] = p
    won = sorted(m.values())
    assert len(dkey) == len(m) and dkey.tolist() == [int(cols[3][p]) for p in won]
    assert srv.tolist() == [int(cols[0][p]) for p in won] and gid.tolist() == [int(cols[1][p]) for p in won]
    assert stid.tolist() == [int(cols[2][p]) for p in won]
    assert cnt.tolist() == [scan(cols, k)[1] for k in dkey.tolist()] and int(cnt.sum()) == n
    assert (srv.dtype, gid.dtype, cnt.dtype) == (np.uint32, np.uint64, np.uint32)


def test_library_and_binding_have_the_two_calls():
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "lib"], cwd=ROOT)
    so = ctypes.CDLL(binding.LIB_PATH)
    for name in ("ydc_stream_book_find", "ydc_stream_book_distinct"):
        assert hasattr(so, name) and name in binding.ABI_SYMBOLS, name
    assert callable(binding.Context.stream_book_find) and callable(binding.Context.stream_book_distinct)
    assert binding.HIT_DTYPE == FM.HIT and binding.HIT_DTYPE.itemsize == 32
    assert binding.BOOK_NOT_FOUND == FM.NOT_FOUND
    assert callable(streaming.find_running)
