"""The byte format of ydc_stream_delta_inspect / ydc_stream_inspect_restore /
ydc_stream_delta_apply_inspected without a GPU.

State pairs come from the lease and rpc models (tests/stream_lease_model.py, stream_rpc_model.py) with
tests/stream_inspect_model.py attached: a model runs some ticks, its state with its inspection records is
A; it runs on, that is B. For every pair the delta sidecar of B's inserted leases is built, parsed and
applied to A's records beside the delta itself, which must give B's records in every column; the full
sidecar of B read alone must give them too; a blob's size is 120 + 8n + 8n + 4n + 4n + pad8(n) + 16 *
n_servants; and the C++ build of yadcc_amd/csrc/stream_inspect_delta_codec.h
(tests/native/inspect_delta_codec_test.cc, ASan + UBSan, given the columns as a file) must give the very
bytes numpy's build_inspect_delta gives. parse_inspect_delta refuses every class of bad blob the C
validator names, and the C validator runs over good blobs and seeded corruptions as a program of its own.
Every test fails without the feature: snapshot.py has no build_inspect_delta and the codec header does
not exist."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import stream_inspect_model as IM
from tests import stream_lease_model as L
from tests import stream_rpc_cases as rcases
from tests import stream_rpc_model as RM
from tests import stream_snapshot_model as SM
from tests.conftest import ROOT
from yadcc_amd import snapshot as S, synth

CAPS = dict(max_updates=300, max_releases=16, max_tasks=1024, max_leases=4096, max_renewals=4096, max_frees=4096,
            max_reports=300, max_report_ids=4096)
FAR = 1 << 40
RECORD = ("task_id", "started_at", "env_id", "requestor_ip", "prefetch")
SERVANT = ("discovered_at", "ever_assigned")
IDENTITY = ("stamp", "next_id", "last_now", "lease_tick", "n_leases", "epoch")


def pool(n, slots):
    sv = synth.make_servants(n, n_tasks_hint=n * slots, n_envs=1, seed=42)
    sv["num_processors"][:], sv["current_load"][:] = 1 << 16, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = slots, 0
    return sv


class Leased:
    """The lease model with hand-made traffic and, from inspect() on, the inspection model on top."""

    def __init__(self, servants=8, slots=512, first_id=0, inspect_now=True):
        self.ls = L.LeaseStream(pool(servants, slots), 0, 0, 0, L.LeaseTable(), n_envs=1)
        self.ls.es.hb = 2
        self.ls.table.next_id = first_id
        self.t, self.I, self.epoch = 0, None, 0
        if inspect_now:
            self.inspect()

    def inspect(self):
        self.I = IM.attach(self.ls)
        self.epoch += 1  # (ydc_stream_inspect_begin)

    def tick(self, n=0, **over):
        ev = dict(self.ls.next_tick())
        none64 = np.empty(0, np.uint64)
        ev.update(renew_ids=none64, renew_expires_at=np.empty(0, np.int64), free_ids=none64,
                  report_servants=np.empty(0, np.uint32), report_off=np.zeros(1, np.uint32), report_ids=none64,
                  tasks=synth.make_tasks(n, self.ls.es.sv, n_envs=1, seed=self.t + 1, self_frac=0.0),
                  release_idx=np.empty(0, np.uint32), lease_expires_at=np.full(n, FAR, np.int64))
        ev.update(over)
        self.t += 1
        want = IM.model_tick(L, self.ls, ev) if self.I is not None else L.model_tick(self.ls, ev)
        assert (want["out"] < L.IDX_ENV_NOT_FOUND).sum() == n, "the pool is too small for this case"
        return want

    def ids(self):
        return np.array(sorted(self.ls.table.L), np.uint64)

    def state(self):
        """-> (the parsed full snapshot, inspect_state())."""
        full = S.parse(S.build(SM.state_of("leased", self.ls, CAPS, self.t)))
        return full, S.inspect_state(full, self.I.tasks(), self.I.servants(), self.epoch)


def leased_pairs():
    out = {}
    m = Leased()
    m.tick(40)
    a = m.state()
    out["no inserts"] = (a, a, 0)
    m.tick(0, free_ids=m.ids()[3:9])
    b = m.state()
    out["no inserts, six erased"] = (a, b, 0)
    for k in (1, 63, 64, 65, 1000):
        before = m.state()
        m.tick(k, free_ids=m.ids()[::3][:k])
        out["%d inserts" % k] = (before, m.state(), k)
    before = m.state()
    ids = m.ids()
    m.tick(0, free_ids=ids)
    m.tick(len(ids))
    out["every lease erased and as many inserted"] = (before, m.state(), len(ids))
    # Leases granted before inspection was switched on: the sentinels.
    z = Leased(inspect_now=False)
    z.tick(30)
    z.inspect()
    a = z.state()
    assert (a[1]["env_id"] == IM.NO_ID).all() and (a[1]["started_at"] == IM.NO_TIME).all()
    z.tick(10, free_ids=z.ids()[:5])
    b = z.state()
    assert (b[1]["env_id"] == IM.NO_ID).sum() == 25 and (b[1]["env_id"] != IM.NO_ID).sum() == 10
    out["sentinels"] = (a, b, 10)
    h = Leased(first_id=1 << 40)
    h.tick(20)
    a = h.state()
    h.tick(20, free_ids=h.ids()[::2])
    b = h.state()
    assert int(b[1]["task_id"].min()) > 1 << 40
    out["ids from 2^40"] = (a, b, 20)
    for n in (1, 63, 64, 65, 257):
        s = Leased(servants=n, slots=64)
        s.tick(20)
        a = s.state()
        s.tick(7, free_ids=s.ids()[:2])
        out["%d servants" % n] = (a, s.state(), 7)
    e = Leased()
    a = e.state()
    assert a[1]["n_leases"] == 0
    e.tick(1)
    b = e.state()
    out["|L| 0 -> 1"] = (a, b, 1)
    e.tick(0, free_ids=e.ids())
    out["|L| 1 -> 0"] = (b, e.state(), 0)
    return out


def rpc_pairs():
    """RPCs with immediate and prefetch rows: the prefetch flag both ways among a delta's inserted leases."""
    ws = rcases.small_stream(max_rows=3000, max_waiting=64)
    caps = dict(CAPS, max_tasks=24, max_rows=3000, max_waiting=64)
    I = IM.attach(ws)
    t = [0]

    def tick(**kw):
        t[0] += 1
        return IM.model_tick(RM, ws, rcases.scripted(ws, ws.next_tick(), **kw))

    def state():
        full = S.parse(S.build(SM.state_of("rpc", ws, caps, t[0])))
        return full, S.inspect_state(full, I.tasks(), I.servants(), 1)

    tick(rpcs=[(2, 1, 10, 20), (1, 0, 10, 20)])
    a = state()
    tick(rpcs=[(1, 2, 10, 20), (3, 0, 11, 20), (0, 2, 12, 20), (2, 3, 13, 20)], free=sorted(ws.state.T.L)[:2])
    b = state()
    new = ~np.isin(b[1]["task_id"], a[1]["task_id"])
    assert set(b[1]["prefetch"][new].tolist()) == {0, 1}, "the inserted leases do not carry the flag both ways"
    return {"rpc, prefetch both ways": (a, b, int(new.sum()))}


def all_pairs():
    if not hasattr(all_pairs, "made"):
        all_pairs.made = dict(leased_pairs(), **rpc_pairs())
    return all_pairs.made


PAIR_NAMES = ["no inserts", "no inserts, six erased", "1 inserts", "63 inserts", "64 inserts", "65 inserts", "1000 inserts",
              "every lease erased and as many inserted", "sentinels", "ids from 2^40", "1 servants", "63 servants",
              "64 servants", "65 servants", "257 servants", "|L| 0 -> 1", "|L| 1 -> 0", "rpc, prefetch both ways"]


def test_the_pairs_are_all_listed():
    assert sorted(all_pairs()) == sorted(PAIR_NAMES)


def promised_size(n, n_servants):
    return 120 + 8 * n + 8 * n + 4 * n + 4 * n + S._pad8(n) + 16 * n_servants


def same_state(got, want):
    for k in IDENTITY:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in RECORD + SERVANT:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_build_parse_and_apply_round_trip(name):
    (fa, a), (fb, b), n_ins = all_pairs()[name]
    delta = S.build_delta(fa, fb)
    d = S.parse_delta(delta)
    assert d["n_ins"] == n_ins
    side = S.build_inspect_delta(b, d["ins_id"], S.INSPECT_DELTA)
    p = S.parse_inspect_delta(side)
    assert (p["kind"], p["n"], p["n_servants"]) == (S.INSPECT_DELTA, n_ins, len(fb["version"]))
    assert np.array_equal(p["task_id"], d["ins_id"])
    assert len(side) == promised_size(n_ins, len(fb["version"]))
    same_state(S.apply_inspect_delta(a, side, delta), b)
    # The full sidecar alone is the state, at |L| of 0 and 1 too.
    full = S.build_inspect_delta(b, None, S.INSPECT_FULL)
    q = S.parse_inspect_delta(full)
    assert (q["kind"], q["n"]) == (S.INSPECT_FULL, b["n_leases"]) and len(full) == promised_size(b["n_leases"], len(fb["version"]))
    same_state(S.apply_inspect_delta(None, full), b)
    # One state, one encoding: built again from what was read, the same bytes.
    assert S.build_inspect_delta(S.apply_inspect_delta(None, full), d["ins_id"], S.INSPECT_DELTA) == side
    # What must not be applied.
    with pytest.raises(S.FormatError):
        S.apply_inspect_delta(a, full, delta)  # (a full sidecar beside a delta)
    with pytest.raises(S.FormatError):
        S.apply_inspect_delta(dict(a, epoch=a["epoch"] + 1), side, delta)  # (records were rewritten on the primary)
    if fa is not fb:
        with pytest.raises(S.FormatError):
            S.apply_inspect_delta(b, side, delta)  # (applied already: the delta's base is gone)
    if n_ins:
        other = S.build_inspect_delta(b, b["task_id"][:1] if b["task_id"][0] != d["ins_id"][0] else b["task_id"][-1:],
                                      S.INSPECT_DELTA)
        if n_ins > 1 or S.parse_inspect_delta(other)["task_id"][0] != d["ins_id"][0]:
            with pytest.raises(S.FormatError):
                S.apply_inspect_delta(a, other, delta)  # (another id column than the delta's inserted list)


def test_build_refuses_an_id_that_is_no_lease():
    _, (fb, b), _ = all_pairs()["64 inserts"]
    for ids in ([b["next_id"] + 3], [int(b["task_id"][0]), b["next_id"]]):
        with pytest.raises(S.FormatError):
            S.build_inspect_delta(b, np.array(ids, np.uint64), S.INSPECT_DELTA)


def sealed(b):
    b = bytearray(b)
    b[24:32] = S.checksum(bytes(b)).to_bytes(8, "little")
    return bytes(b)


F = dict(kind=32, n_servants=36, n=40, reserved=44, stamp=48, next_id=56, last_now=64, lease_tick=72, n_leases=76, epoch=80,
         dir=88)


def bad_blobs(blob, full):
    """One blob per check of the validator, by name; `blob` a delta sidecar of >= 3 records whose record
    section is padded, `full` a full one."""
    d = S.parse_inspect_delta(blob)
    n, ns = d["n"], d["n_servants"]
    assert n >= 3 and n % 8 and d["n_leases"] > n
    for k, at in F.items():  # (the offsets above are the header's)
        if k != "dir":
            width = 4 if k in ("kind", "n_servants", "n", "reserved", "lease_tick", "n_leases") else 8
            assert int.from_bytes(blob[at:at + width], "little", signed=k == "last_now") == d[k], k
    rec, srv = 120, 120 + S._pad8(25 * n)
    assert struct.unpack_from("<4Q", blob, F["dir"]) == (rec, srv - rec, srv, 16 * ns)

    def put(at, value, width=4, of=blob):
        out = bytearray(of)
        out[at:at + width] = (int(value) % (1 << (8 * width))).to_bytes(width, "little")
        return sealed(out)

    def u64(at):
        return int.from_bytes(blob[at:at + 8], "little")

    return {
        "cut inside the header": blob[:100],
        "cut inside a section": blob[:rec + 20],
        "one byte short": blob[:-1],
        "eight bytes short": blob[:-8],
        "a byte behind": blob + b"\0",
        "eight zero bytes behind, sealed": sealed(blob + bytes(8)),
        "flipped byte in the header": blob[:50] + bytes([blob[50] ^ 1]) + blob[51:],
        "flipped byte in the records": blob[:rec + 5] + bytes([blob[rec + 5] ^ 0x80]) + blob[rec + 6:],
        "flipped byte in the servants": blob[:srv + 9] + bytes([blob[srv + 9] ^ 2]) + blob[srv + 10:],
        "a forged checksum": blob[:24] + bytes([blob[24] ^ 1]) + blob[25:],
        "not a sidecar": put(0, S.DELTA_MAGIC, 8),
        "unknown version": put(8, 2),
        "header size": put(12, 128),
        "total bytes": put(16, len(blob) + 8, 8),
        "unknown kind": put(F["kind"], 2),
        "reserved set": put(F["reserved"], 1),
        "a tick number whose stamp is 0": put(F["lease_tick"], 1 << 30),
        "more records than leases": put(F["n_leases"], n - 1),
        "a full sidecar of fewer records than |L|": put(F["kind"], 0),
        "a full sidecar, |L| off by one": put(F["n_leases"], S.parse_inspect_delta(full)["n_leases"] + 1, of=full),
        "more leases than ids": put(F["next_id"], d["n_leases"] - 1, 8),
        "n + 1": put(F["n"], n + 1),
        "n 2^32 - 1": put(F["n"], 0xFFFFFFFF),
        "n_servants + 1": put(F["n_servants"], ns + 1),
        "n_servants 2^32 - 1": put(F["n_servants"], 0xFFFFFFFF),
        "section offset moved": put(F["dir"] + 16, srv + 8, 8),
        "section size 2^63": put(F["dir"] + 8, 1 << 63, 8),
        "ids not ascending": put(rec + 8, u64(rec), 8),
        "ids descending": put(rec, u64(rec + 8) + 1, 8),
        "an id == next_id": put(rec + 8 * (n - 1), d["next_id"], 8),
        "an id 2^64 - 1": put(rec + 8 * (n - 1), (1 << 64) - 1, 8),
        "prefetch 2": put(rec + 24 * n + 1, 2, 1),
        "prefetch 255": put(rec + 24 * n + n - 1, 255, 1),
        "padding not zero": put(rec + 25 * n, 1, 1),
        "the last padding byte not zero": put(srv - 1, 0x80, 1),
    }


def test_parse_refuses_corruptions():
    _, (fb, b), _ = all_pairs()["rpc, prefetch both ways"]
    _, (_, bl), _ = all_pairs()["65 inserts"]
    blob = S.build_inspect_delta(bl, bl["task_id"][-13:], S.INSPECT_DELTA)
    full = S.build_inspect_delta(b, None, S.INSPECT_FULL)
    for name, bytes_ in bad_blobs(blob, full).items():
        with pytest.raises(S.FormatError):
            S.parse_inspect_delta(bytes_)
            pytest.fail("%s was accepted" % name)
    assert S.parse_inspect_delta(sealed(blob))["n"] == 13


@pytest.fixture(scope="module")
def codec_tool(tmp_path_factory):
    """tests/native/inspect_delta_codec_test.cc: includes only the codec headers; ASan + UBSan, built the
    way test_stream_delta_codec.py builds its twin, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inspect_delta_codec") / "inspect_delta_codec_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "inspect_delta_codec_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_c_validator_under_sanitizers(codec_tool):
    out = subprocess.run([codec_tool], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "INSPECT-CODEC-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_c_validator_refuses_what_numpy_refuses(codec_tool, tmp_path):
    _, (fb, b), _ = all_pairs()["rpc, prefetch both ways"]
    _, (_, bl), _ = all_pairs()["65 inserts"]
    blob = S.build_inspect_delta(bl, bl["task_id"][-13:], S.INSPECT_DELTA)
    path = str(tmp_path / "blob.bin")
    for name, bytes_ in bad_blobs(blob, S.build_inspect_delta(b, None, S.INSPECT_FULL)).items():
        open(path, "wb").write(bytes_)
        assert subprocess.run([codec_tool, "check", path], capture_output=True, timeout=120).returncode == 1, name
    open(path, "wb").write(blob)
    assert subprocess.run([codec_tool, "check", path], capture_output=True, timeout=120).returncode == 0


def column_file(state, ids, kind):
    """The input of the tool's build: nine u64 words, then the seven columns unpadded."""
    ids = state["task_id"] if kind == S.INSPECT_FULL else np.asarray(ids, np.uint64)
    at = np.searchsorted(state["task_id"], ids)
    head = [kind, len(state["discovered_at"]), len(ids), state["stamp"], state["next_id"], state["last_now"] % (1 << 64),
            state["lease_tick"], state["n_leases"], state["epoch"]]
    return (np.array(head, "<u8").tobytes() + b"".join(np.ascontiguousarray(state[c][at]).tobytes() for c in RECORD) +
            b"".join(np.ascontiguousarray(state[c]).tobytes() for c in SERVANT))


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_c_and_numpy_build_the_same_bytes(name, codec_tool, tmp_path):
    (fa, a), (fb, b), _ = all_pairs()[name]
    ins = S.parse_delta(S.build_delta(fa, fb))["ins_id"]
    fc, fo = str(tmp_path / "columns.bin"), str(tmp_path / "side.bin")
    for kind in (S.INSPECT_DELTA, S.INSPECT_FULL):
        open(fc, "wb").write(column_file(b, ins, kind))
        r = subprocess.run([codec_tool, "build", fc, fo], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(fo, "rb").read() == S.build_inspect_delta(b, ins, kind), "the C++ and the numpy build disagree (kind %d)" % kind
        assert subprocess.run([codec_tool, "check", fo], capture_output=True, timeout=120).returncode == 0
