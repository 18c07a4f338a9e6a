"""Cost of ydc_stream_delta_inspect and ydc_stream_delta_apply_inspected beside ydc_stream_delta and
ydc_stream_delta_apply (unchanged by the sidecars: timed in the same run as the yardstick), at
stream_delta_cost.py's shape and with its method: 2000 servants (cfg5), 10k requests, 10k frees by id, 200
heartbeats, 200 reports and 2k renewals per tick over about --leases ballast leases; medians of --reps,
one process. Each size is a step of its own, under its own time limit, the next one only behind it:
    timeout -k 10 300 python tests/tools/stream_delta_inspect_cost.py --leases 40000 --reps 9 && \\
    timeout -k 10 600 python tests/tools/stream_delta_inspect_cost.py --leases 1020000 --reps 9
A primary with inspection on, the ballast in and 20 ticks behind it takes a base and the full sidecar. Two
standbys are restored from the base: one without inspection, which applies every delta with
ydc_stream_delta_apply, and one with ydc_stream_inspect_restore, which applies every pair with
ydc_stream_delta_apply_inspected. Then --reps times: one tick on the primary, ydc_stream_delta,
ydc_stream_delta_inspect (both into buffers that are large enough: one call each), and the two applies;
the same with ten ticks between the deltas and with none. Prints one JSON line, wall time from host call
to host return. Nothing is asserted about a time. Needs the GPU."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import stream_snapshot_cost as base  # noqa: E402
from yadcc_amd import binding, pack, snapshot, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS, E64, E32, FAR, timed = base.N, base.HB_REPORTS, base.RENEWALS, base.E64, base.E32, base.FAR, base.timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leases", type=int, default=40_000)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    max_leases = a.leases + 4 * N
    ctx = binding.Context(device=0)
    ctx.upload_servants(pack.to_abi_columns(sv))
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, max_leases, RENEWALS, N, HB_REPORTS, 1 << 16)
    ctx.stream_inspect_begin()
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
    for _ in range(20):
        traffic.tick(ctx)
    C, lib = binding.C, binding.lib()
    blob = ctx.stream_delta_base()
    full_ms, full_side = timed(ctx.stream_delta_inspect)  # (two calls: the size, then the bytes)
    plain, inspected = binding.Context(device=0), binding.Context(device=0)
    plain.stream_restore(blob)
    inspected.stream_restore(blob)
    restore_ms, _ = timed(lambda: inspected.stream_inspect_restore(full_side))
    cap = len(blob) + (1 << 16)
    buf, side_buf, need = C.create_string_buffer(cap), C.create_string_buffer(cap), C.c_size_t(0)

    def delta():
        rc = lib.ydc_stream_delta(ctx._h, buf, C.c_size_t(cap), C.byref(need))
        assert rc == 0, (rc, lib.ydc_last_error(ctx._h))
        return C.string_at(buf, need.value)  # (not buf.raw[:n], which copies the whole buffer first)

    def sidecar(d):
        rc = lib.ydc_stream_delta_inspect(ctx._h, d, C.c_size_t(len(d)), side_buf, C.c_size_t(cap), C.byref(need))
        assert rc == 0, (rc, lib.ydc_last_error(ctx._h))
        return C.string_at(side_buf, need.value)

    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    res = {}
    for name, ticks in (("1", 1), ("10", 10), ("0", 0)):
        t = dict(delta_ms=[], delta_inspect_ms=[], apply_ms=[], apply_inspected_ms=[])
        size, side_size, inserted = [], [], 0
        for _ in range(a.reps):
            for _ in range(ticks):
                traffic.tick(ctx)
            ms, d = timed(delta)
            t["delta_ms"].append(ms)
            ms, s = timed(lambda: sidecar(d))
            t["delta_inspect_ms"].append(ms)
            t["apply_ms"].append(timed(lambda: plain.stream_delta_apply(d))[0])
            t["apply_inspected_ms"].append(timed(lambda: inspected.stream_delta_apply_inspected(d, s))[0])
            size.append(len(d))
            side_size.append(len(s))
            inserted = snapshot.DELTA_HEADER.unpack_from(d)[28]
            assert len(s) == 120 + 24 * inserted + snapshot._pad8(inserted) + 16 * len(sv["version"])
        res["delta_%s_ticks" % name] = dict(bytes=int(np.median(size)), sidecar_bytes=int(np.median(side_size)), inserted=inserted,
                                            **{k: med(v) for k, v in t.items()})
    full = ctx.stream_snapshot()
    assert plain.stream_snapshot() == full and inspected.stream_snapshot() == full, "a standby fell out of step"
    tp, ts = ctx.stream_inspect_tasks(), inspected.stream_inspect_tasks()
    assert all(np.array_equal(tp[k], ts[k]) for k in tp), "the standby's records are not the primary's"
    n_l = len(tp["task_id"])
    for c in (ctx, plain, inspected):
        c.stream_end()
        c.close()
    print(json.dumps(dict(res, leases=n_l, n_servants=len(sv["version"]), snapshot_bytes=len(full), reps=a.reps,
                          full_sidecar_bytes=len(full_side), full_sidecar_ms=round(full_ms, 3),
                          inspect_restore_ms=round(restore_ms, 3))))


if __name__ == "__main__":
    main()
