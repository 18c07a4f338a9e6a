"""The byte format of ydc_stream_snapshot / ydc_stream_restore without a GPU: yadcc_amd/snapshot.py
(build / parse) on hand-made states of every mode and on corruptions of their blobs, and the C
validator (yadcc_amd/csrc/stream_snapshot_codec.h) as a stand-alone ASan + UBSan program
(tests/native/snapshot_codec_test.cc) on good blobs and several hundred seeded corruptions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from yadcc_amd import snapshot as S

CAPS = dict(max_updates=16, max_releases=8, max_tasks=48)
LEASE_CAPS = dict(max_leases=64, max_renewals=16, max_frees=16, max_reports=4, max_report_ids=32)


def registry(n, env_words=1, seed=1):
    rng = np.random.default_rng(seed)
    d = {k: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for k in S.REGISTRY_U32}
    d["env_mask"] = rng.integers(0, 1 << 63, (n, env_words), dtype=np.uint64)
    return d


def leases(n_l, n, next_id=None, seed=2):
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 9, n_l)).astype(np.uint64) + np.uint64(1 << 40)
    return dict(leased=True, l_id=ids, l_expires_at=rng.integers(-5, 1000, n_l).astype(np.int64),
                l_servant=rng.integers(0, max(n, 1), n_l).astype(np.uint32), l_zombie=(rng.random(n_l) < 0.3).astype(np.uint8),
                l_stamp=rng.integers(0, 1 << 30, n_l).astype(np.uint32),
                next_id=int(ids[-1]) + 1 if n_l and next_id is None else next_id or 0, lease_tick=77, **LEASE_CAPS)


def waiting(n_w, leased, rpc, seed=3):
    rng = np.random.default_rng(seed)
    d = dict(waiting=True, max_waiting=32, w_deadline=rng.integers(0, 99, n_w).astype(np.int64),
             w_tag=rng.integers(0, 1 << 60, n_w).astype(np.uint64), w_env_id=rng.integers(0, 64, n_w).astype(np.uint32),
             w_min_version=rng.integers(0, 4, n_w).astype(np.uint32),
             w_requestor_ip=rng.integers(0, 1 << 32, n_w, dtype=np.uint64).astype(np.uint32))
    if leased:
        d["w_lease_for"] = rng.integers(1, 50, n_w).astype(np.int64)
    if rpc:
        d.update(rpc=True, max_rows=200, w_n_immediate=rng.integers(0, 4, n_w).astype(np.uint32),
                 w_n_prefetch=rng.integers(1, 3, n_w).astype(np.uint32))
    return d


def states():
    n = 7
    book = dict(book=True, max_book=40, b_grant_id=np.arange(5, dtype=np.uint64) + np.uint64(1 << 41),
                b_servant_task_id=np.arange(5, dtype=np.uint64) * np.uint64(3), b_digest_key=np.full(5, 2 ** 63 + 5, np.uint64),
                b_servant=np.array([0, 6, 6, 2, 1], np.uint32))
    alive = dict(alive=True, e_expires_at=np.array([50, S.I64_MAX, 12, 13, 12, 900, 77], np.int64))
    return {
        "waiting": dict(CAPS, **registry(n), **waiting(5, False, False), last_now=3),
        "leased": dict(CAPS, **registry(n), **leases(9, n), last_now=-4),
        "leased, wide masks, aliases": dict(CAPS, **registry(n, 2), **leases(1, n), alias_ip=np.array([9, 8], np.uint32),
                                            alias_servant=np.array([6, 0], np.uint32)),
        "leased, empty": dict(CAPS, **registry(0), **leases(0, 0)),
        "waiting and leased": dict(CAPS, **registry(n), **leases(4, n), **waiting(3, True, False)),
        "rpc": dict(CAPS, **registry(n), **leases(6, n), **waiting(4, True, True)),
        "rpc, book, alive": dict(CAPS, **registry(n, 3), **leases(11, n), **waiting(2, True, True), **book, **alive),
        "leased, alive": dict(CAPS, **registry(n), **leases(3, n), **alive),
    }


@pytest.mark.parametrize("name", sorted(states()))
def test_build_parse_round_trip(name):
    want = states()[name]
    blob = S.build(want)
    got = S.parse(blob)
    assert len(blob) % 8 == 0 and S.build(got) == blob, "parse -> build changed the bytes"
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    for mode, _ in S.MODE_BITS:
        assert got[mode] == bool(want.get(mode))
    if want.get("leased"):
        assert np.array_equal(got["l_state"], np.uint32(S.LIVE) | (want["l_zombie"].astype(np.uint32) << np.uint32(30)) | want["l_stamp"])
    assert got["alive_bound"] == (12 if want.get("alive") else S.I64_MAX)
    assert got["last_now"] == want.get("last_now", S.I64_MIN)
    assert got["n_wait_rows"] == (int(want["w_n_immediate"].sum() + want["w_n_prefetch"].sum()) if want.get("rpc") else 0)


def sealed(b):
    b = bytearray(b)
    b[24:32] = S.checksum(bytes(b)).to_bytes(8, "little")
    return bytes(b)


def test_parse_refuses_corruptions():
    blob = S.build(states()["rpc, book, alive"])
    head = S.HEADER.unpack_from(blob)
    off = {name: head[28 + 2 * k] for k, name in enumerate(("registry", "L", "W", "B", "E"))}
    n_l = head[20]

    def put(at, value, width=4):
        b = bytearray(blob)
        b[at:at + width] = int(value).to_bytes(width, "little")
        return sealed(b)

    bad = {
        "cut at the header": blob[:100],
        "cut inside a section": blob[:off["L"] + 20],
        "one byte short": blob[:-1],
        "eight bytes short": blob[:-8],
        "a byte behind": blob + b"\0",
        "flipped byte in the header": blob[:41] + bytes([blob[41] ^ 1]) + blob[42:],
        "flipped byte in L": blob[:off["L"] + 5] + bytes([blob[off["L"] + 5] ^ 0x80]) + blob[off["L"] + 6:],
        "ids not ascending": put(off["L"] + 8, int.from_bytes(blob[off["L"]:off["L"] + 8], "little"), 8),
        "id >= next_id": put(off["L"] + 8 * (n_l - 1), head[25], 8),
        "servant index >= n_servants": put(off["L"] + 16 * n_l, 7),
        "lease without the live bit": put(off["L"] + 20 * n_l, 5),
        "unknown version": put(8, 2),
        "n_servants + 1": put(40, 8),
        "|L| + 1": put(92, n_l + 1),
        "|L| beyond max_leases": put(92, 1000),
        "rows(W) off by one": put(100, head[22] + 1),
        "book entry on no servant": put(off["B"] + 24 * 5, 7),
        "E below alive_bound": put(off["E"], 11, 8),
        "section offset moved": put(136 + 16, off["L"] + 8, 8),
        "section size 2^63": put(136 + 24, 1 << 63, 8),
        "mode without the book": put(32, head[5] & ~8),
        "env_words 0": put(36, 0),
        "not a snapshot": put(0, 0x1122334455667788, 8),
    }
    for name, b in bad.items():
        with pytest.raises(S.FormatError):
            S.parse(b)
            pytest.fail("%s was accepted" % name)
    with pytest.raises(S.FormatError):
        S.build(dict(states()["leased"], l_servant=np.zeros(3, np.uint32)))


def test_c_validator_under_sanitizers(tmp_path):
    """tests/native/snapshot_codec_test.cc: includes only the codec header; ASan + UBSan, built the way
    the sanitizer programs of tests/native/Makefile are, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "snapshot_codec_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "snapshot_codec_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SNAPSHOT-CODEC-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
