"""The fair-share level's model (tests/stream_fair_model.py) on the CPU: the yardstick of
tests/test_stream_fair_gpu.py.

The closed form (bisection) against the literal progressive fill on a seeded sweep; the hand vector of
include/yadcc_dispatch.h's rule; every boundary of the rule; and on seeded saturated 12-servant streams
in both modes the defining property: a second stream with the STATIC quota, given tick by tick the
default the level came to, answers identically — through the quota model and, where oracle/_ref is built,
through the verbatim reference class on the clipped requests. The invariant after every tick; a pool
nobody can fill changes nothing; the constants against the header."""
import os
import re

import numpy as np
import pytest

from tests import stream_fair_model as F
from tests import stream_quota_model as Q
from tests import stream_wait_lease_model as WL
from tests import test_stream_quota_model as TQ
from tests.conftest import ROOT
from yadcc_amd import binding

UNL = F.UNLIMITED
A, B, C_ = TQ.A, TQ.B, TQ.C_
HAND = [(0, 10, None), (3, 10, None), (8, 4, None)]


# ---- the arithmetic ---------------------------------------------------------------------------------

def test_closed_form_is_the_progressive_fill():
    rng = np.random.default_rng(11)
    seen = {"unl": 0, "zero": 0, "mid": 0, "none": 0}
    for _ in range(12000):
        n = int(rng.integers(0, 7))
        askers = []
        for _ in range(n):
            h, a = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            askers.append((h, a, int(rng.integers(0, 40)) if rng.random() < 0.25 else None))
        others, pool = int(rng.integers(0, 40)), int(rng.integers(0, 160))
        lv = F.level(askers, others, pool)
        assert lv == F.fill(askers, others, pool), (askers, others, pool)
        fair = [x for x in askers if x[2] is None]
        seen["none" if not fair else "unl" if lv == UNL else "zero" if lv == 0 else "mid"] += 1
        if fair and lv != UNL:  # the written rule, checked directly
            D = max(h + a for h, a, _ in fair)
            assert lv < D and F.f_at(askers, others, lv + 1) > pool
            assert F.f_at(askers, others, lv) <= pool or (lv == 0 and F.f_at(askers, others, 0) > pool)
    assert min(seen.values()) > 300, seen


def test_the_hand_vector():
    assert [F.f_at(HAND, 2, lv) for lv in range(7)] == [13, 14, 15, 16, 18, 20, 22]
    assert F.level(HAND, 2, 20) == 5 == F.fill(HAND, 2, 20)
    ips = [A] * 1 + [B] * 1 + [C_] * 1
    a_imm, a_pre = Q.clip(ips, [10, 10, 4], [0, 0, 0], {A: 0, B: 3, C_: 8}, lambda ip: 5)
    assert list(a_imm) == [5, 2, 0] and not a_pre.any()
    # (the remainder: 20 - f(5) = 0 here; at P = 21 one row stays free, less than one per asker above the level)
    assert F.level(HAND, 2, 21) == 5 and F.f_at(HAND, 2, 5) == 20


def test_boundaries_of_the_level():
    D = 13  # max(h + a)
    fD, f0 = F.f_at(HAND, 2, D), F.f_at(HAND, 2, 0)
    assert (fD, f0) == (2 + 10 + 13 + 12, 13)
    assert F.level(HAND, 2, fD) == UNL          # f(D) == P: all demand fits
    assert F.level(HAND, 2, fD - 1) == D - 1    # f(D) == P + 1: the largest level below D
    assert F.f_at(HAND, 2, D - 1) == fD - 1
    assert F.level(HAND, 2, f0) == 0            # f(0) == P
    assert F.level(HAND, 2, f0 - 1) == 0        # f(0) == P + 1
    assert F.level(HAND[1:], 0, 11) == 3        # f(0) == P and the levels below everybody's h add nothing: f(3) == 11 < f(4)
    assert [F.f_at(HAND, 5, lv) for lv in range(5)] == [16, 17, 18, 19, 21]
    assert F.level(HAND, 5, 16) == 0            # f(0) == P, f(1) > P
    assert F.level(HAND, 5, 15) == 0            # f(0) == P + 1
    assert F.level(HAND, 2, 0) == 0
    assert F.level([], 7, 0) == UNL             # no asker at all
    assert F.level([(1, 5, 3), (0, 9, 0)], 7, 0) == UNL  # no FAIR asker
    # a saturating pool: P is at most 2^32 - 2, so a level below D never reaches YDC_QUOTA_UNLIMITED
    big = [((1 << 32) - 2, (1 << 32) - 2, None), (0, 5, None)]
    assert F.level(big, 0, 1 << 40) == F.level(big, 0, F.POOL_MAX) == 0  # (f(0) = 2^32 - 2 = P; f(1) = P + 1)
    assert F.level([(0, (1 << 32) - 2, None)], 0, 1 << 40) == UNL
    assert F.level([(0, (1 << 32) - 1, None)], 0, 1 << 40) == F.POOL_MAX
    assert F.pool_of((1 << 40), 100) == F.POOL_MAX and F.pool_of(199, 50) == 99 and F.pool_of(3, 150) == 4


def test_overrides_above_and_below_the_level():
    # an override is a fixed term at its own cap, whatever the level
    base = [(0, 10, None), (3, 10, None)]
    assert F.level(base + [(8, 4, 20)], 2, 32) == F.level(base, 2 + 12, 32) == 9   # above the level: takes h + a
    assert F.level(base + [(8, 4, 2)], 2, 32) == F.level(base, 2 + 8, 32) == 12    # below it: keeps what it holds
    assert F.level(base + [(8, 4, 9)], 2, 32) == F.level(base, 2 + 9, 32)


def test_the_cap_from_the_level():
    assert F.cap_default(5, 0, UNL) == 5 and F.cap_default(5, 3, UNL) == 5 and F.cap_default(2, 3, UNL) == 3
    assert F.cap_default(0, 0, UNL) == 0 and F.cap_default(0, 3, 2) == 2
    assert F.cap_default(UNL, 3, 40) == 40 and F.cap_default(9, 0, 4) == 4  # default_cap below the level
    q = Q.Quota(WL, None)
    q.begin(4)
    q.set(7, {C_: 9})
    f = F.Fair(q)
    ips, want = [A, A, B, C_], [4, 6, 10, 4]
    held = {A: 0, B: 3, C_: 8}
    for percent, P, lv, eff in ((50, 9, 0, 0), (100, 18, 3, 3), (150, 27, 8, 7)):
        f.fair(F.REGISTRY, percent, 0)
        r = f.evaluate(held, 13, 18, ips, want)  # O = 2; C_ is an override: fixed min(12, 9) = 9
        assert (r["pool"], r["level"], r["cap_default_effective"]) == (P, lv, eff), (percent, r)
        assert (r["n_askers"], r["n_override_askers"], r["held_others"], r["asked_rows"]) == (3, 1, 2, 24)
    f.fair(F.FIXED, 18, 5)
    assert f.evaluate(held, 13, 999, ips, want)["cap_default_effective"] == 5  # the floor above the level
    f.fair(F.FIXED, 1 << 32, 0)
    assert f.evaluate(held, 13, 999, ips, want)["pool"] == F.POOL_MAX
    with pytest.raises(ValueError):
        f.fair(F.REGISTRY, 0)
    with pytest.raises(ValueError):
        f.fair(3, 1)


def test_top_is_the_slot_count_at_running_zero():
    assert F.top(8, 0, 4, 0) == 4 and F.top(2, 1, 4, 1) == 2
    assert F.top(8, 8, 4, 0) == 0 and F.top(8, 9, 4, 0) == 0 and F.top(8, 0, 0, 0) == 0 and F.top(8, 0, 4, 2) == 0
    assert F.top(8, 0, 4, 3) == 0


# ---- the defining property on seeded streams ------------------------------------------------------------

CAPS = (7, {A: 9, C_: 2})
FAIRS = {"registry": (F.REGISTRY, 150), "fixed": (F.FIXED, 22)}  # (the pool has 18 slots)


def _run_fair(mode, fair, floor=0, caps=CAPS, ticks=28):
    """-> (labelled records, base records, clips, effective defaults, levels)."""
    ws = TQ.new_stream(mode)
    q = Q.Quota(TQ.MODS[mode], ws)
    q.begin(4)
    q.set(*caps)
    f = F.Fair(q)
    f.fair(fair[0], fair[1], floor)
    rng, rec, base, clips, eff, levels = np.random.default_rng(7), [], [], [], [], []
    for t in range(ticks):
        ev = TQ.few_requestors(ws.next_tick(), rng)
        r = f.tick(ev)
        if floor == 0:
            assert f.invariant(), (t, f.level_result)
        for x in (r, q.base):
            x["next_id"] = ws.table.next_id
            x["rows_w"] = ws.state.q.rows() if mode == "rpc" else len(ws.state.q)
        rec.append(r)
        base.append(q.base)
        clips.append(q.result)
        eff.append(f.effective)
        levels.append(f.level_result["level"])
    return rec, base, clips, eff, levels


def _run_static(mode, eff, caps=CAPS):
    """The second stream: the static quota, its default_cap set tick by tick."""
    ws = TQ.new_stream(mode)
    q = Q.Quota(TQ.MODS[mode], ws)
    q.begin(4)
    rng, rec = np.random.default_rng(7), []
    for e in eff:
        q.set(e, caps[1])
        r = q.tick(TQ.few_requestors(ws.next_tick(), rng))
        r["next_id"] = ws.table.next_id
        r["rows_w"] = ws.state.q.rows() if mode == "rpc" else len(ws.state.q)
        rec.append(r)
    return rec


@pytest.mark.parametrize("pool", sorted(FAIRS))
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property(mode, pool):
    rec, base, clips, eff, levels = _run_fair(mode, FAIRS[pool])
    # the level is at work: ticks at a level of its own, ticks where all fits, requests refused
    assert sum(1 for lv in levels if lv != UNL) > 8 and UNL in levels, levels
    assert sum(c[3] for c in clips) > 20 and min(eff) < 7 and len(set(eff)) > 2, eff
    TQ._same(mode, rec, _run_static(mode, eff), "the static quota given the level's default")
    want, _, _ = TQ._run(mode, clips=clips)
    TQ._same(mode, base, want, "the base model on the clipped requests")


@TQ.needs_ref
@pytest.mark.parametrize("pool", sorted(FAIRS))
@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_defining_property_against_the_reference_replay(mode, pool):
    rec, base, clips, eff, levels = _run_fair(mode, FAIRS[pool])
    want, _, _ = TQ._run(mode, clips=clips, replay=True)
    TQ._same(mode, base, want, "the verbatim class on the clipped requests")


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_a_floor_and_other_percents_keep_the_property(mode):
    for fair, floor in (((F.REGISTRY, 50), 3), ((F.REGISTRY, 100), 0)):
        rec, base, clips, eff, levels = _run_fair(mode, fair, floor=floor, ticks=16)
        assert all(e >= min(floor, 7) for e in eff)
        TQ._same(mode, rec, _run_static(mode, eff), "the static quota given the level's default")


@pytest.mark.parametrize("mode", ["wl", "rpc"])
def test_a_pool_nobody_fills_is_the_quota_alone(mode):
    rec, _, clips, eff, levels = _run_fair(mode, (F.FIXED, (1 << 32) - 1))
    assert set(levels) == {UNL} and set(eff) == {7}
    want, _, _ = TQ._run(mode, caps=CAPS)
    TQ._same(mode, rec, want, "the quota-only model")


def test_mode_off_is_the_quota_model():
    rec, _, _, eff, _ = _run_fair("wl", (F.OFF, 0), ticks=10)
    want, _, _ = TQ._run("wl", caps=CAPS, ticks=10)
    TQ._same("wl", rec, want, "mode off")
    assert set(eff) == {None}


# ---- the header -----------------------------------------------------------------------------------------

def test_abi_carries_the_fair_level():
    assert (binding.FAIR_OFF, binding.FAIR_REGISTRY, binding.FAIR_FIXED) == (F.OFF, F.REGISTRY, F.FIXED) == (0, 1, 2)
    src = open(os.path.join(ROOT, "include", "yadcc_dispatch.h")).read()
    assert re.search(r"#define YDC_ABI_VERSION 8u", src)
    for name, v in (("OFF", 0), ("REGISTRY", 1), ("FIXED", 2)):
        assert re.search(r"#define YDC_FAIR_%s %du" % (name, v), src), name
    for name in ("ydc_stream_quota_fair", "ydc_stream_quota_fair_result", "ydc_fair_level"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.ABI_SYMBOLS
    assert hasattr(binding.Context, "stream_quota_fair") and hasattr(binding.Context, "stream_quota_fair_result")
    m = re.search(r"typedef struct \{([^}]*)\} ydc_fair_result;", src)
    fields = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert tuple(f for f in fields if not f.startswith("uint")) == F.RESULT_FIELDS
    assert tuple(k for k, _ in binding.FairResult._fields_) == F.RESULT_FIELDS
    hdr = open(os.path.join(ROOT, "yadcc_amd", "csrc", "fair_level.h")).read()
    assert re.search(r"kFairPoolMax = 0xFFFFFFFEull", hdr) and F.POOL_MAX == 0xFFFFFFFE
    dev = open(os.path.join(ROOT, "yadcc_amd", "csrc", "stream_fair.h")).read()
    assert re.search(r"kFairPerThread = 16;", dev) and re.search(r"kFairRegAskers = kFairThreads \* kFairPerThread", dev)
