#!/usr/bin/env python3
"""What two device lanes can win on cfg2, measured without them: two contexts on one device are
two streams with two workspaces. One host thread times three loops of bench.py's cfg2 step (same
synth calls, same DeviceArrays, no COMMIT):
  (a) one context, two batches in flight (bench.py's loop; YDC_TUNE=lanes=0: on one lane)
  (b) two contexts, one batch in flight each: async(A), async(B), wait(A), wait(B)
  (c) two contexts, two batches in flight each
and prints one JSON line with the aggregate ms per batch of each and, per context, what
ydc_debug_pipeline counts (profiles/lanes_ceiling_cfg2.txt: the library before it had lanes).
usage: python tools/lanes_probe.py [cfg2] [steps] [warmup]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yadcc_amd import binding, pack, synth  # noqa: E402


class Lane:
    """One context with bench.py's buffers: the request columns and two pairs of result arrays."""

    def __init__(self, sv, tk):
        DA = binding.DeviceArray
        self.ctx = binding.Context(device=0)
        self.ctx.upload_servants(pack.to_abi_columns(sv))
        self.cols = [DA.from_numpy(tk[k]) for k in ("env_id", "min_version", "requestor_ip")]
        n_tasks, n_serv = len(tk["env_id"]), len(sv["version"])
        self.res = [(DA(n_tasks, np.uint32), DA(n_serv, np.uint32)) for _ in range(2)]
        self.k = 0

    def send(self):
        out, run = self.res[self.k & 1]
        self.k += 1
        self.ctx.dispatch_device_async(self.cols[0], self.cols[1], self.cols[2], out, None, run)

    def wait(self):
        self.ctx.dispatch_wait()


def loop_a(A, k):
    """bench.py's run_steps: k batches, two in flight."""
    A.send()
    for _ in range(1, k):
        A.send()
        A.wait()
    A.wait()


def loop_b(A, B, k):
    """k batches over two contexts, one in flight on each."""
    for _ in range(k // 2):
        A.send()
        B.send()
        A.wait()
        B.wait()


def loop_c(A, B, k):
    """k batches over two contexts, two in flight on each."""
    A.send()
    B.send()
    for _ in range(1, k // 2):
        A.send()
        B.send()
        A.wait()
        B.wait()
    A.wait()
    B.wait()


def timed(fn, lanes, steps, warmup):
    fn(*lanes, warmup)
    for ln in lanes:
        ln.ctx.synchronize()
    t0 = time.perf_counter()
    fn(*lanes, steps)
    for ln in lanes:
        ln.ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    n_cfg, s_cfg, n_envs, unk = synth.CONFIGS[cfg]
    sv = synth.make_servants(s_cfg, n_tasks_hint=n_cfg, n_envs=n_envs, seed=42, shared_ip_frac=0.0)
    tk = synth.make_tasks(n_cfg, sv, n_envs=n_envs, unknown_env_frac=unk)
    A, B = Lane(sv, tk), Lane(sv, tk)
    rec = {"config": cfg, "steps": steps, "warmup": warmup,
           "a_one_context_two_deep_ms": timed(loop_a, (A,), steps, warmup),
           "b_two_contexts_one_deep_ms": timed(loop_b, (A, B), steps, warmup),
           "c_two_contexts_two_deep_ms": timed(loop_c, (A, B), steps, warmup)}
    # (batches placed, of them enqueued on the context's own second lane, placed again after a miss)
    rec["debug_pipeline"] = [list(ln.ctx.debug_pipeline()) for ln in (A, B)]
    # (both contexts must have placed what one context places: the same registry, the same batch)
    rec["same_placement"] = bool(np.array_equal(A.res[0][0].numpy(), B.res[0][0].numpy())
                                 and np.array_equal(A.res[0][0].numpy(), A.res[1][0].numpy()))
    print(json.dumps(rec))
    A.ctx.close()
    B.ctx.close()


if __name__ == "__main__":
    main()
