"""Cost of ydc_stream_snapshot and ydc_stream_restore beside ydc_stream_leases_get (the way out that
existed before, and the yardstick), and the first tick after a restore beside an ordinary tick, at
lease_tick_cost.py's shape: 2000 servants (cfg5), 10k requests, 10k frees by id, 200 heartbeats, 200
reports and 2k renewals per tick over about --leases ballast leases.
    python tests/tools/stream_snapshot_cost.py --leases 100000 --reps 9
One leased stream with the ballast in and 20 measured ticks behind it; then, in the same process,
--reps times each: ydc_stream_leases_get, ydc_stream_snapshot, ydc_stream_restore into a second
context (which is ended again) — and once more a restore whose context then runs the next ticks:
its first tick (it captures its step) and the median of the following ones. Prints one JSON line
with the medians, wall time from host call to host return. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS = 10_000, 200, 2_000
E64, E32 = np.empty(0, np.uint64), np.empty(0, np.uint32)
FAR = 1 << 40


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


class Traffic:
    """lease_tick_cost.py's tick, one after another, on whichever context it is handed."""

    def __init__(self, sv, held):
        self.es = streaming.EventStream(sv, N, 0)
        self.rng = np.random.default_rng(5)
        self.held, self.t = held, 0
        self.live_ids, self.live_srv = E64, E32

    def tick(self, ctx):
        es, t = self.es, self.t
        now = t + 1
        who, rows, _, tk = es.next_tick()
        ren = self.rng.integers(0, max(self.held, 1), RENEWALS).astype(np.uint64)  # ballast ids: live, never freed
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % es.n).astype(np.uint32)
        order = np.argsort(self.live_srv, kind="stable")
        srt = self.live_srv[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([self.live_ids[order[a:b]] for a, b in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        lex = np.full(len(tk["env_id"]), now + 5, np.int64)
        ms, (out, ids, _, _, n_l) = timed(lambda: ctx.stream_tick_leased(
            who, rows, E32, ren, np.full(RENEWALS, FAR, np.int64), self.live_ids, rs, off, rid, tk, lex, now))
        g = out < binding.IDX_ENV_NOT_FOUND
        self.live_ids, self.live_srv = ids[g], out[g]
        self.t += 1
        return ms, int(n_l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ticks", type=int, default=40)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    abi = pack.to_abi_columns(sv)
    max_leases = a.leases + 4 * N
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    held = 0
    while held < a.leases:  # ballast: leases nobody frees; their slots go back by servant index
        who, rows, _, tk = es.next_tick()
        n = min(N, a.leases - held)
        tk = {k: v[:n] for k, v in tk.items()}
        out, ids, _, _, held = ctx.stream_tick_leased(who, rows, E32, E64, E64.view(np.int64), E64, E32,
                                                      np.zeros(1, np.uint32), E64, tk, np.full(n, FAR, np.int64), 0)
        g = out[out < binding.IDX_ENV_NOT_FOUND]
        ctx.stream_tick_leased(E32, rows[:0], g, E64, E64.view(np.int64), E64, E32, np.zeros(1, np.uint32), E64,
                               {k: v[:0] for k, v in tk.items()}, E64.view(np.int64), 0)
    traffic = Traffic(sv, held)
    traffic.es = es
    before = [traffic.tick(ctx)[0] for _ in range(20 + a.ticks)][20:]
    get, snap, rest = [], [], []
    blob = b""
    for _ in range(a.reps):
        get.append(timed(ctx.stream_leases)[0])
        ms, blob = timed(ctx.stream_snapshot)
        snap.append(ms)
        other = binding.Context(device=0)
        rest.append(timed(lambda: other.stream_restore(blob))[0])
        other.stream_end()
        other.close()
    n_l = len(ctx.stream_leases()[0])
    ctx.stream_end()
    ctx.close()
    fresh = binding.Context(device=0)
    fresh.stream_restore(blob)
    first, _ = traffic.tick(fresh)
    after = [traffic.tick(fresh)[0] for _ in range(a.ticks)]
    fresh.stream_end()
    fresh.close()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    print(json.dumps({"leases": n_l, "slots": max(1024, 1 << int(np.ceil(np.log2(2 * max_leases)))), "blob_bytes": len(blob),
                      "reps": a.reps, "leases_get_ms": med(get), "snapshot_ms": med(snap), "restore_ms": med(rest),
                      "tick_before_ms": med(before), "first_tick_after_restore_ms": round(first, 3),
                      "tick_after_restore_ms": med(after)}))


if __name__ == "__main__":
    main()
