"""What looking a digest up in the running-task book costs: a leased stream over
cfg5's registry whose book holds --entries distinct keys (one lease, listed that many times by its
servant with the keys staged: an id listed k times gives k entries), and --queries digests, half of
them in the book. In one process, alternating, medians of --repeats after a warm-up:
  find_rebuild   ydc_stream_book_find on a stale index: table cleared, k_book_index_build,
                 k_book_index_find, the results copied back. (A tick with an empty report of an
                 idle servant, not timed, makes the index stale and leaves B as it is.)
  find           the same call on a valid index: k_book_index_find and the copies;
  distinct       ydc_stream_book_distinct on a valid index: k_book_distinct and five columns back;
  host_*         what a scheduler has without the calls: ydc_stream_book_get (host_get), then a map
                 from digest_key to the last entry built on the host and the queries asked of it —
                 with numpy (a stable argsort and two searchsorted: host_numpy) and with a Python
                 dict (host_dict). Each includes host_get.
Then --ticks ticks of the same stream (2000 requests, 2000 frees by id, heartbeats, no reports),
alternately with a find (not timed) in front of the tick and without: tick and tick_after_find.
    python tests/tools/book_find_cost.py
prints one JSON line, times in microseconds of wall time from host call to host return (every call
ends in a device synchronise). Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, LIFE, FAR = 2_000, 10, 1 << 40
E64, E32 = np.empty(0, np.uint64), np.empty(0, np.uint32)
ODD = np.uint64(0x9E3779B97F4A7C15)  # (odd: k -> k * ODD is a bijection of the 64-bit keys)


class Stream:
    def __init__(self, entries):
        sv, _ = synth.make_config("cfg5")
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(pack.to_abi_columns(sv))
        self.es = streaming.EventStream(sv, N, 0)
        self.ctx.stream_begin_leased(self.es.hb + 8, N, N, (LIFE + 4) * N, 16, N, 16, entries)
        self.ctx.stream_book_begin(entries)
        self.live, self.now = [], 0

    def tick(self, reports=(), keys=None):
        """One tick: heartbeats, N requests that live LIFE ticks, the frees of those that are over,
        reports: [(servant, [id])] with `keys` staged. -> (seconds, out, ids)."""
        self.now += 1
        who, rows, rel, tk = self.es.next_tick()
        fr = self.live.pop(0) if len(self.live) == LIFE else E64
        rs = np.array([s for s, _ in reports], np.uint32)
        off = np.cumsum([0] + [len(i) for _, i in reports]).astype(np.uint32)
        rid = np.concatenate([np.asarray(i, np.uint64) for _, i in reports]) if reports else E64
        lex = np.full(len(tk["env_id"]), FAR, np.int64)
        if keys is not None:
            self.ctx.stream_book_stage(None, keys)
        t0 = time.perf_counter()
        out, ids, _, unknown, _ = self.ctx.stream_tick_leased(who, rows, rel, E64, np.empty(0, np.int64), fr, rs, off,
                                                              rid, tk, lex, self.now)
        el = time.perf_counter() - t0
        assert not unknown.any()
        self.es.commit(out)
        g = out < binding.IDX_ENV_NOT_FOUND
        self.live.append(ids[g])
        return el, out[g], ids[g]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def host_numpy(cols, q):
    """digest_key -> its last entry, by a stable sort; the queries by binary search."""
    srv, _, stid, dkey = cols
    order = np.argsort(dkey, kind="stable")
    srt = dkey[order]
    hi = np.searchsorted(srt, q, side="right")
    hit = (hi > 0) & (srt[np.maximum(hi, 1) - 1] == q)
    last = order[np.maximum(hi, 1) - 1]
    return hit, srv[last], stid[last]


def host_dict(cols, q):
    """The reference's pass (running_task_keeper.cc:55-60) and its TryFindTask, in Python."""
    srv, _, stid, dkey = cols
    m = {}
    for k, s, t in zip(dkey.tolist(), srv.tolist(), stid.tolist()):
        m[k] = (s, t)
    return [m.get(k) for k in q.tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--ticks", type=int, default=200)
    a = ap.parse_args()
    s = Stream(a.entries)
    ctx = s.ctx
    _, out, ids = s.tick()
    held, tid = int(out[0]), int(ids[0])
    s.live[0] = s.live[0][1:]  # (this lease stays: its servant lists it --entries times)
    keys = np.arange(a.entries, dtype=np.uint64) * np.uint64(2) * ODD
    s.tick(reports=[(held, [tid] * a.entries)], keys=keys)
    assert len(ctx.stream_book()[0]) == a.entries
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.choice(keys, a.queries // 2),
                        (rng.integers(0, 1 << 40, a.queries - a.queries // 2, dtype=np.uint64) * np.uint64(2)
                         + np.uint64(1)) * ODD])
    rng.shuffle(q)
    idle = (held + 1) % s.es.n
    T = {k: [] for k in ("find_rebuild", "find", "distinct", "host_get", "host_numpy", "host_dict")}
    for r in range(a.repeats + 5):
        s.tick(reports=[(idle, [])])
        dt, (hits, built) = timed(lambda: ctx.stream_book_find(q))
        assert built and int((hits["pos"] != binding.BOOK_NOT_FOUND).sum()) == a.queries // 2
        T["find_rebuild"].append(dt)
        dt, (again, built) = timed(lambda: ctx.stream_book_find(q))
        assert not built and np.array_equal(again, hits)
        T["find"].append(dt)
        dt, (fold, built) = timed(ctx.stream_book_distinct)
        assert not built and len(fold[0]) == a.entries
        T["distinct"].append(dt)
        dt_get, cols = timed(ctx.stream_book)
        T["host_get"].append(dt_get)
        dt, (hit, srv, stid) = timed(lambda: host_numpy(cols, q))
        assert np.array_equal(hit, hits["pos"] != binding.BOOK_NOT_FOUND)
        assert np.array_equal(stid[hit], hits["servant_task_id"][hit]) and np.array_equal(srv[hit], hits["servant_idx"][hit])
        T["host_numpy"].append(dt_get + dt)
        if r % 8 == 0:  # (seconds each: a few are enough)
            dt, found = timed(lambda: host_dict(cols, q))
            assert [f is not None for f in found] == hit.tolist()
            T["host_dict"].append(dt_get + dt)
    plain, asked = [], []
    for t in range(a.ticks + 20):
        if t % 2:
            _, built = ctx.stream_book_find(q)
            assert not built
        (asked if t % 2 else plain).append(s.tick()[0])
    med = lambda x, skip: round(float(np.median(x[skip:])) * 1e6, 1)
    res = {"entries": a.entries, "queries": a.queries, "repeats": a.repeats, "ticks": a.ticks}
    res.update({k + "_us": med(v, 5 if k != "host_dict" else 1) for k, v in T.items()})
    res.update(tick_us=med(plain, 10), tick_after_find_us=med(asked, 10))
    print(json.dumps(res))
    ctx.stream_end()
    ctx.close()


if __name__ == "__main__":
    main()
