"""The rings of a matching wave at small class counts, on the device against the oracle: the size the
plan takes on its own (2048 entries) and rings sized to the batch — 256 entries per class up to 8
classes, 512 .. 2048 in all, forced with YDC_RING_TOTAL. Sized rings were measured and not made
the default (NOTES_rejected.md 7.1: no faster beside a batch on the other lane); the switch stays,
and these tests say that it only ever was a question of speed: 1, 2, 3, 4, 5, 8 and 9 classes with
chunks of 64 and 128 requests, pools in which one class supplies several hundred consecutive picks
(a 256-entry ring has to be topped up inside a chunk, and by the waves that follow a chain of
chunks), and requests from the servants' own hosts — holes in the order — with two servants on one
host."""
import functools

import numpy as np
import pytest

from oracle import oraclebind as O
from tests import cases, class_edge_cases as K
from yadcc_amd import binding, pack, synth

pytestmark = pytest.mark.gpu

CLASS_COUNTS = (1, 2, 3, 4, 5, 8, 9)
CHUNKS = (64, 128)


def with_classes(sv, n_classes, seed):
    """The pool with its servants dealt into n_classes classes at random: class c has version
    19 + (c & 1) and digest set (c >> 1) + 1 (digests 0 .. 2)."""
    n = len(sv["version"])
    cls = np.random.default_rng(seed).integers(0, n_classes, n)
    cls[:n_classes] = np.arange(n_classes)  # (every class exists)
    sv = dict(sv)
    sv["version"] = (19 + (cls & 1)).astype(np.uint32)
    sv["env_mask"] = ((cls >> 1) + 1).astype(np.uint64)
    sv["max_tasks"] = np.maximum(sv["max_tasks"], 1).astype(np.uint32)  # (every servant takes tasks)
    return sv


@functools.lru_cache(maxsize=None)
def class_case(n_classes):
    n_tasks = 8000 + 1500 * n_classes  # 9.5k .. 21.5k: another number of chunks for every class count
    sv = with_classes(synth.make_servants(400, n_tasks_hint=n_tasks, n_envs=1, seed=40 + n_classes), n_classes,
                      seed=n_classes)
    tk = synth.make_tasks(n_tasks, sv, n_envs=3 if n_classes > 1 else 1, seed=140 + n_classes, self_frac=0.1,
                          unknown_env_frac=0.002)
    assert K.plan_of(sv, n_tasks)["C"] == n_classes
    return sv, tk, O.dispatch(sv, tk, "sorted")


def sized(n_classes):
    """Rings sized to the batch: the smallest power of two >= 256 entries per class (what keeps the
    level-table fill of few-class batches, match_kernel.h), 512 at least, 2048 at most."""
    t = 512
    while t < 2048 and t < 256 * n_classes:
        t *= 2
    return t


RINGS = ("plan", "sized")


def run(monkeypatch, sv, tk, want, chunk, rings, **switches):
    """One batch on a fresh context with a forced chunk size and the replay counter on, the rings as
    the plan chooses or sized to the class count. Equal to the oracle; returns the stats."""
    monkeypatch.delenv("YDC_RING_TOTAL", raising=False)
    if rings == "sized":
        switches = dict(switches, RING_TOTAL=sized(K.plan_of(sv, len(tk["env_id"]))["C"]))
    for k, v in dict(CHUNK_SIZE=chunk, DEBUG_SIM=1, **switches).items():
        monkeypatch.setenv("YDC_" + k, str(v))
    c = binding.Context(device=0)
    try:
        c.upload_servants(pack.to_abi_columns(sv))
        got, gutil, grun = c.dispatch(tk)
        st = c.stats()
    finally:
        c.close()
    idx, util, wrun = want
    bad = np.nonzero(got != idx)[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], idx[bad[:5]], st)
    assert np.array_equal(gutil, util) and np.array_equal(grun, wrun), st
    assert st["n_chunks"] == -(-len(idx) // chunk) and st["small_batch"] == 0, st
    return st


@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_rings_by_class_count(monkeypatch, n_classes, chunk, rings):
    sv, tk, want = class_case(n_classes)
    st = run(monkeypatch, sv, tk, want, chunk, rings)
    print("classes %d chunk %d rings %s: n_chunks %d chunk_sims %d rounds %d" % (
        n_classes, chunk, rings, st["n_chunks"], st["chunk_sims"], st["rounds"]))
    assert st["n_classes"] == n_classes and st["radix_passes"] == 0, st


@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n_classes", (2, 4))
def test_rings_with_the_radix_sort(monkeypatch, n_classes, chunk, rings):
    """The same rings behind the radix sort (no level table: the waves search the class lists)."""
    sv, tk, want = class_case(n_classes)
    st = run(monkeypatch, sv, tk, want, chunk, rings, BINSORT=0)
    assert st["radix_passes"] >= 1, st


def longest_run(values):
    """Longest stretch of equal consecutive values."""
    v = np.asarray(values)
    if v.size == 0:
        return 0
    cut = np.flatnonzero(np.concatenate(([True], v[1:] != v[:-1], [True])))
    return int(np.diff(cut).max())


@functools.lru_cache(maxsize=None)
def one_class_ahead(n_classes):
    """Class 0: 60 idle servants of 64 processors; the other classes: 30 servants each, half taken.
    Every request may go to every class, so the order of the slots decides alone: the idle class
    supplies every pick until it is as loaded as the others — far more than a ring of 256."""
    n_rest = 30 * (n_classes - 1)
    n = 60 + n_rest
    sv = synth.make_servants(n, n_tasks_hint=4000, n_envs=1, seed=17)
    sv["version"][:] = 20
    sv["num_processors"][:] = 64
    sv["max_tasks"][:] = 60
    sv["current_load"][:] = 0
    sv["running_tasks"][:60] = 0
    sv["running_tasks"][60:] = 30
    sv["priority"][:] = 2
    sv["total_memory"][:] = 64 << 30
    sv["memory_available"][:] = 32 << 30
    cls = np.concatenate([np.zeros(60, np.int64), 1 + np.arange(n_rest) % max(1, n_classes - 1)])
    sv["env_mask"] = (np.uint64(1) | (cls.astype(np.uint64) << np.uint64(1)))  # digest 0 everywhere
    tk = synth.make_tasks(8000, sv, n_envs=1, seed=18, self_frac=0.0, min_version_20_frac=0.0)
    want = O.dispatch(sv, tk, "sorted")
    placed = want[0][want[0] < O.IDX_ENV_NOT_FOUND]
    assert K.plan_of(sv, 8000)["C"] == n_classes
    assert longest_run(cls[placed]) > 600, longest_run(cls[placed])  # (several rings of 256, many chunks)
    return sv, tk, want


@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("chunk", (64, 128, 192))
@pytest.mark.parametrize("n_classes", (2, 3, 4))
def test_one_class_supplies_hundreds_of_consecutive_picks(monkeypatch, n_classes, chunk, rings):
    """Chunks of 192: a wave's first fill is 128 entries, so it tops its ring up inside the chunk;
    every chunk size: the chunks of the stretch start where a predecessor's ring would long have
    wrapped."""
    sv, tk, want = one_class_ahead(n_classes)
    st = run(monkeypatch, sv, tk, want, chunk, rings)
    assert st["n_classes"] == n_classes and st["radix_passes"] == 0, st


@functools.lru_cache(maxsize=None)
def holes_case(n_classes):
    sv, _ = cases.random_case(seed=50 + n_classes, n_tasks=10_000, n_servants=300, n_envs=1, shared_ip_frac=0.25)
    sv = with_classes(sv, n_classes, seed=7 * n_classes)
    tk = synth.make_tasks(10_000, sv, n_envs=3, seed=250 + n_classes, self_frac=0.3)
    assert len(np.unique(sv["ip"])) < len(sv["ip"])  # two servants on one host
    return sv, tk, O.dispatch(sv, tk, "sorted")


@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n_classes", (2, 4, 8))
def test_own_hosts_and_shared_hosts(monkeypatch, n_classes, chunk, rings):
    """A third of the requests come from servants' own hosts (they may not take their own slots: the
    chunk hands a state with holes on) and a quarter of the servants share a host with an earlier one."""
    sv, tk, want = holes_case(n_classes)
    st = run(monkeypatch, sv, tk, want, chunk, rings)
    assert st["n_classes"] == n_classes, st
