"""What the servants' expiry adds to a leased tick, at lease_tick_cost.py's shape:
cfg5's registry, 10k requests, 10k frees by id, 200 heartbeats, 2k renewals and 200 reports per
tick; a grant lives ten ticks. In one process, fed the same ticks:
  plain     the leased tick without aliveness;
  alive     the same tick with aliveness on, every heartbeat far in the future: the step plus
            k_alive_beat, never an alarm;
  alarm     every tick's first heartbeat renews a servant whose old expiry is behind the clock, so
            the host's bound is low, k_alive_due is launched and finds nobody: the alarm that ends
            empty, in every tick;
  removal   every `--every`-th tick one servant (the last row) runs out: the eager heartbeats, the
            compaction, the tables rebuilt, the step captured again, k_alive_orphans. The median of
            those ticks alone is reported, and the same servant is appended again two ticks later
            (a structural tick that is not counted);
  remove_by_caller   what a caller without aliveness pays for the same: ydc_remove_servants of the
            last row followed by a tick (captured again), every `--every`-th tick.
    python tests/tools/alive_tick_cost.py --ticks 300
prints one JSON line: the median wall time per tick (host call to host return, the staging call
included) of every run, two runs each, alternating. Needs the GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from yadcc_amd import binding, pack, streaming, synth  # noqa: E402

N, HB_REPORTS, RENEWALS, LIFE = 10_000, 200, 2_000, 10
E64 = np.empty(0, np.uint64)
FAR = 1 << 40


def run(sv, abi, ticks, kind, every):
    ctx = binding.Context(device=0)
    ctx.upload_servants(abi)
    es = streaming.EventStream(sv, N, 0)
    ctx.stream_begin_leased(es.hb + 8, N, N, (LIFE + 4) * N, RENEWALS, N, HB_REPORTS, 1 << 16)
    alive = kind in ("alive", "alarm", "removal")
    n0 = es.n
    if alive:
        ctx.stream_alive_begin(np.full(n0, FAR, np.int64))
    last = {k: v[n0 - 1:n0].copy() for k, v in abi.items() if isinstance(v, np.ndarray) and len(v) == n0}
    rng = np.random.default_rng(5)
    live = []  # (ids, servants) of the last LIFE ticks' grants
    dt, special = [], []
    n_rows = n0  # rows of the registry on the device
    for t in range(ticks + 20):
        now = t + 1
        who, rows, rel, tk = es.next_tick()
        keep = who < n_rows
        who, rows = who[keep], rows[keep]
        exp = np.full(len(who), FAR, np.int64)
        phase = (t - 20) % every if t >= 20 and kind in ("removal", "remove_by_caller") else -1
        if phase == 2 and n_rows == n0 - 1:  # the servant comes back: appended again
            row = np.zeros(1, dtype=binding.ROW_DTYPE)
            for k in ("version", "num_processors", "current_load", "max_tasks", "flags", "ip_id", "env_mask"):
                row[k] = last[k]
            who, rows, exp = np.append(who, np.uint32(n0 - 1)), np.concatenate([rows, row]), np.append(exp, FAR)
            n_rows = n0
        if kind == "alarm" and len(who):
            exp[0] = FAR - 1000 + now  # (it was given now - 1 below: the bound is behind the clock)
        fr = live.pop(0)[0] if len(live) == LIFE else E64
        ids_all = np.concatenate([a for a, _ in live]) if live else E64
        srv_all = np.concatenate([b for _, b in live]) if live else np.empty(0, np.uint32)
        ren = rng.choice(ids_all, RENEWALS) if len(ids_all) else E64
        rs = ((t * HB_REPORTS + np.arange(HB_REPORTS)) % (n0 - 1)).astype(np.uint32)
        order = np.argsort(srv_all, kind="stable")
        srt = srv_all[order]
        lo, hi = np.searchsorted(srt, rs), np.searchsorted(srt, rs, side="right")
        rid = np.concatenate([ids_all[order[l:h]] for l, h in zip(lo, hi)]) if len(order) else E64
        off = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint32)
        lex = np.full(len(tk["env_id"]), now + 4 * LIFE, np.int64)
        if kind == "alarm" and len(who):
            col = ctx.stream_alive()
            col[who[0]] = now - 1
            ctx.stream_alive_begin(col)
        if kind == "removal" and phase == 0 and n_rows == n0:
            col = ctx.stream_alive()
            col[n0 - 1] = now - 1
            ctx.stream_alive_begin(col)
            keep = who != n0 - 1
            who, rows, exp = who[keep], rows[keep], exp[keep]
        t0 = time.perf_counter()
        if kind == "remove_by_caller" and phase == 0 and n_rows == n0:
            ctx.remove_servants(np.array([n0 - 1], np.uint32))
            n_rows = n0 - 1
            keep = who != n0 - 1
            who, rows, exp = who[keep], rows[keep], exp[keep]
        if alive:
            ctx.stream_alive_stage(exp)
        out, ids, _, unknown, n_l = ctx.stream_tick_leased(who, rows, rel, ren, np.full(len(ren), now + 4 * LIFE, np.int64),
                                                           fr, rs, off, rid, tk, lex, now)
        el = time.perf_counter() - t0
        if kind == "removal" and phase == 0 and n_rows == n0:
            assert list(ctx.stream_alive_removed()[0]) == [n0 - 1]
            n_rows = n0 - 1
        (special if phase == 0 else dt).append(el)
        # (the stream's own view keeps every row; grants on the row that is away cannot happen)
        es.commit(out)
        g = out < binding.IDX_ENV_NOT_FOUND
        live.append((ids[g], out[g]))
    extra = ctx.debug_alive() if alive else None
    ctx.stream_end()
    ctx.close()
    med = lambda a: round(float(np.median(a)) * 1e6, 1) if len(a) else None
    return med(special if kind in ("removal", "remove_by_caller") else dt[20:]), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--kinds", default="plain,alive,alarm,removal,remove_by_caller")
    a = ap.parse_args()
    sv, _ = synth.make_config("cfg5")
    # (the last row idle and never asked for: its leaving changes no placement)
    abi = pack.to_abi_columns(sv)
    res = {"ticks": a.ticks, "every": a.every}
    for kind in a.kinds.split(",") * 2:
        us, extra = run(sv, abi, a.ticks, kind, a.every)
        res.setdefault(kind + "_tick_us", []).append(us)
        if extra:
            res[kind + "_bound_alarms_removed"] = list(extra)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
