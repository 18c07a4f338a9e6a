"""Cost of ydc_stream_delta and ydc_stream_delta_apply beside ydc_stream_snapshot and ydc_stream_restore
(unchanged by the deltas: timed in the same run as the yardstick), at stream_snapshot_cost.py's shape
and with its method: 2000 servants (cfg5), 10k requests, 10k frees by id, 200 heartbeats, 200 reports
and 2k renewals per tick over about --leases ballast leases; medians of --reps, one process.
    python tests/tools/stream_delta_cost.py --leases 110000 --reps 9
A primary with the ballast in and 20 ticks behind it takes a base; a standby is restored from it. Then
--reps times: one tick on the primary, ydc_stream_delta into a buffer that is large enough (one call),
ydc_stream_delta_apply on the standby; the same with ten ticks between the deltas; a delta right behind
another (nothing changed: the two passes, the structure stamp and the whole columns alone); and
ydc_stream_snapshot / ydc_stream_restore. At the end the standby ticks: its first tick (it captures its
step) and the median of the following ones beside the primary's. Prints one JSON line, wall time from
host call to host return. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import stream_snapshot_cost as base  # noqa: E402
from yadcc_amd import binding, pack, snapshot, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS, E64, E32, FAR, timed = base.N, base.HB_REPORTS, base.RENEWALS, base.E64, base.E32, base.FAR, base.timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=30_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    max_leases = a.leases + 4 * N
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
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
    traffic = base.Traffic(sv, held)
    traffic.es = es
    before = [traffic.tick(ctx)[0] for _ in range(20 + a.ticks)][20:]
    C, lib = binding.C, binding.lib()
    blob = ctx.stream_delta_base()
    standby = binding.Context(device=0)
    standby.stream_restore(blob)
    cap = len(blob) + (1 << 16)
    buf, need = C.create_string_buffer(cap), C.c_size_t(0)

    def delta():
        rc = lib.ydc_stream_delta(ctx._h, buf, C.c_size_t(cap), C.byref(need))
        assert rc == 0, (rc, lib.ydc_last_error(ctx._h))
        return buf.raw[:need.value]

    res = {}
    for name, ticks in (("1", 1), ("10", 10), ("0", 0)):
        take, apply_, size, lists = [], [], [], None
        for _ in range(a.reps):
            for _ in range(ticks):
                traffic.tick(ctx)
            ms, d = timed(delta)
            take.append(ms)
            apply_.append(timed(lambda: standby.stream_delta_apply(d))[0])
            size.append(len(d))
            h = snapshot.DELTA_HEADER.unpack_from(d)
            lists = dict(inserted=h[28], erased=h[29], updated=h[30])
        res["delta_%s_ticks" % name] = dict(bytes=int(np.median(size)), delta_ms=round(float(np.median(take)), 3),
                                            apply_ms=round(float(np.median(apply_)), 3), **lists)
    assert standby.stream_snapshot() == ctx.stream_snapshot(), "the standby fell out of step"
    snap, rest = [], []
    for _ in range(a.reps):
        ms, full = timed(ctx.stream_snapshot)
        snap.append(ms)
        other = binding.Context(device=0)
        rest.append(timed(lambda: other.stream_restore(full))[0])
        other.stream_end()
        other.close()
    tick_with_base = [traffic.tick(ctx)[0] for _ in range(a.ticks)]
    standby.stream_delta_apply(delta())  # (in step again: the traffic goes on where the primary stops)
    n_l = len(ctx.stream_leases()[0])
    ctx.stream_end()
    ctx.close()
    first, _ = traffic.tick(standby)
    after = [traffic.tick(standby)[0] for _ in range(a.ticks)]
    standby.stream_end()
    standby.close()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    print(json.dumps(dict(res, leases=n_l, n_servants=len(sv["version"]), snapshot_bytes=len(full), reps=a.reps,
                          snapshot_ms=med(snap), restore_ms=med(rest), tick_before_ms=med(before),
                          tick_with_base_ms=med(tick_with_base), first_tick_after_apply_ms=round(first, 3),
                          tick_after_apply_ms=med(after))))


if __name__ == "__main__":
    main()
