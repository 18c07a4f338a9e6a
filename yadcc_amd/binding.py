"""ctypes binding of yadcc_amd/libydc.so (include/yadcc_dispatch.h).

The library is the product; this file only marshals numpy / torch buffers. If the
shared object is missing or no GPU is present every entry point raises — there
is no CPU fallback on purpose.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (YDC_LIB: a measurement build of the same library, e.g. libydc_probe.so — tools/phase_probe.py)
LIB_PATH = os.environ.get("YDC_LIB") or os.path.join(_HERE, "libydc.so")

ABI_VERSION = 8
IPC_HANDLE_BYTES = 256
TRANSPORT_NONE, TRANSPORT_RCCL, TRANSPORT_LOCAL, TRANSPORT_IPC_DEVICE, TRANSPORT_IPC_HOST = range(5)
TRANSPORT_NAMES = ("none", "rccl", "local", "ipc", "ipc-host")
IDX_TIMEOUT = 0xFFFFFFFF
IDX_ENV_NOT_FOUND = 0xFFFFFFFE
IDX_WAITING = 0xFFFFFFFD  # streaming waiting mode: queued on the device, answered in a later tick
IDX_WITHDRAWN = 0xFFFFFFFC  # resolved lists only: the waiting request was withdrawn by its tag
IDX_OVER_QUOTA = 0xFFFFFFFB  # streams with a quota only: the new request was admitted nothing (its requestor is at its cap)
QUOTA_UNLIMITED = 0xFFFFFFFF  # stream_quota_set: no cap
FAIR_OFF, FAIR_REGISTRY, FAIR_FIXED = 0, 1, 2  # stream_quota_fair: the pool's mode (percent of the registry / rows)
INSPECT_NO_ID = 0xFFFFFFFF  # env_id / requestor_ip of a lease granted while inspection was off
INSPECT_NO_TIME = -(1 << 63)  # ... its started_at
OUTLOOK_UNKNOWN = 0xFFFFFFFF  # leases / zombies of an outlook row while inspection is off
BOOK_NOT_FOUND = 0xFFFFFFFF  # pos of a ydc_book_hit whose digest_key is not in the book
REQUESTOR_UNKNOWN = 0xFFFFFFFF  # lease columns of a ydc_requestor_load while inspection is off or without leases
DISPATCH_COMMIT = 1
STAGES = ("servant_scan", "slot_gen", "sort", "class_lists", "task_classify", "match", "finalize",
          "total")

# Every symbol include/yadcc_dispatch.h declares (tests check they are all exported).
ABI_SYMBOLS = (
    "ydc_strerror", "ydc_last_error", "ydc_abi_version", "ydc_create", "ydc_destroy",
    "ydc_upload_servants", "ydc_update_servants", "ydc_update_servants_wide",
    "ydc_set_host_aliases", "ydc_remove_servants", "ydc_release_slots", "ydc_release_slots_device", "ydc_set_running",
    "ydc_get_running", "ydc_dispatch", "ydc_dispatch_tick", "ydc_dispatch_device", "ydc_dispatch_device_async",
    "ydc_dispatch_wait", "ydc_synchronize",
    "ydc_set_profiling", "ydc_get_stats", "ydc_kernel_profile", "ydc_device_count",
    "ydc_device_malloc", "ydc_device_free", "ydc_memcpy_h2d", "ydc_memcpy_d2h",
    "ydc_host_register", "ydc_host_unregister", "ydc_host_alloc", "ydc_host_free",
    "ydc_stream_begin", "ydc_stream_tick", "ydc_stream_tick_wide", "ydc_stream_buffers_get", "ydc_stream_end",
    "ydc_stream_begin_waiting", "ydc_stream_tick_waiting", "ydc_stream_waiting_take",
    "ydc_stream_begin_leased", "ydc_stream_tick_leased", "ydc_stream_leases_get",
    "ydc_stream_begin_waiting_leased", "ydc_stream_tick_waiting_leased",
    "ydc_stream_begin_rpc", "ydc_stream_tick_rpc", "ydc_stream_caps_get", "ydc_stream_reserve",
    "ydc_stream_book_begin", "ydc_stream_book_stage", "ydc_stream_book_get",
    "ydc_stream_book_find", "ydc_stream_book_distinct",
    "ydc_stream_alive_begin", "ydc_stream_alive_stage", "ydc_stream_alive_removed", "ydc_stream_alive_get",
    "ydc_stream_inspect_begin", "ydc_stream_inspect_load", "ydc_stream_inspect_servants", "ydc_stream_inspect_tasks",
    "ydc_stream_outlook_get", "ydc_stream_inspect_waiting",
    "ydc_stream_inspect_select", "ydc_stream_inspect_count",
    "ydc_stream_requestor_find", "ydc_stream_requestor_get", "ydc_admit_clip",
    "ydc_stream_withdraw_begin", "ydc_stream_withdraw_stage", "ydc_stream_withdraw_result",
    "ydc_stream_quota_begin", "ydc_stream_quota_set", "ydc_stream_quota_result",
    "ydc_stream_quota_fair", "ydc_stream_quota_fair_result", "ydc_fair_level",
    "ydc_stream_depart_begin", "ydc_stream_depart_stage", "ydc_stream_depart_result",
    "ydc_stream_usage_begin", "ydc_stream_usage_get", "ydc_stream_usage_find", "ydc_stream_usage_load", "ydc_usage_quanta",
    "ydc_stream_snapshot", "ydc_stream_restore",
    "ydc_stream_delta_base", "ydc_stream_delta", "ydc_stream_delta_apply", "ydc_stream_delta_stop",
    "ydc_stream_delta_inspect", "ydc_stream_inspect_restore", "ydc_stream_delta_apply_inspected",
    "ydc_group_unique_id", "ydc_group_init", "ydc_group_init_local", "ydc_group_destroy",
    "ydc_group_size", "ydc_group_ipc_export", "ydc_group_init_ipc", "ydc_group_transport",
    "ydc_dispatch_sharded",
    # host class wrapper (yadcc_amd/dispatcher.py types them)
    "ydc_td_create", "ydc_td_destroy", "ydc_td_device_status", "ydc_td_set_clock_ns",
    "ydc_td_keep_servant_alive", "ydc_td_wait_for_starting_new_task",
    "ydc_td_wait_for_starting_new_tasks", "ydc_td_keep_task_alive", "ydc_td_free_task",
    "ydc_td_free_tasks", "ydc_td_host_stats", "ydc_td_running_tasks_acquire", "ydc_td_running_tasks_release",
    "ydc_td_notify_servant_running_tasks", "ydc_td_get_running_tasks",
    "ydc_td_on_expiration_timer", "ydc_td_dump_internals", "ydc_td_oplog_enable", "ydc_td_oplog_take",
    "ydc_td_alias_renumbered_turns",
)


class ServantSoA(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("version", "num_processors", "current_load",
                                           "max_tasks", "running_tasks", "flags", "env_mask",
                                           "ip_id")] + [("env_words", C.c_uint32)]


class StreamTotals(C.Structure):
    """ydc_stream_totals."""
    _fields_ = [(k, C.c_uint64) for k in ("servants_up", "running_tasks", "capacity", "capacity_available",
                                          "capacity_unavailable")]


# ydc_lease_filter's `fields` bits (YDC_SEL_*), by the keyword Context.stream_inspect_select takes.
SEL_SERVANT, SEL_ZOMBIE, SEL_EXPIRES_BEFORE, SEL_AFTER_ID = 0x001, 0x002, 0x004, 0x008
SEL_ENV, SEL_REQUESTOR, SEL_PREFETCH, SEL_STARTED_BEFORE, SEL_UNATTRIBUTED = 0x010, 0x020, 0x040, 0x080, 0x100
SELECT_MAX_FILTERS = 64


class LeaseFilter(C.Structure):
    """ydc_lease_filter."""
    _fields_ = [("fields", C.c_uint32), ("servant_idx", C.c_uint32), ("env_id", C.c_uint32),
                ("requestor_ip", C.c_uint32), ("zombie", C.c_uint8), ("prefetch", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("expires_before", C.c_int64), ("started_before", C.c_int64), ("after_id", C.c_uint64)]


def lease_filter(servant=None, zombie=None, expires_before=None, after_id=None, env_id=None, requestor_ip=None,
                 prefetch=None, started_before=None, unattributed=False):
    """A LeaseFilter from keywords: a predicate takes part when its keyword is not None (unattributed:
    when true). Values are checked by the library, not here, except that they must fit their member."""
    f = LeaseFilter()
    for bit, name, v in ((SEL_SERVANT, "servant_idx", servant), (SEL_ZOMBIE, "zombie", zombie),
                         (SEL_EXPIRES_BEFORE, "expires_before", expires_before), (SEL_AFTER_ID, "after_id", after_id),
                         (SEL_ENV, "env_id", env_id), (SEL_REQUESTOR, "requestor_ip", requestor_ip),
                         (SEL_PREFETCH, "prefetch", prefetch), (SEL_STARTED_BEFORE, "started_before", started_before)):
        if v is None:
            continue
        v = int(v)
        lo, hi = {"zombie": (0, 255), "prefetch": (0, 255), "expires_before": (-2**63, 2**63 - 1),
                  "started_before": (-2**63, 2**63 - 1), "after_id": (0, 2**64 - 1)}.get(name, (0, 2**32 - 1))
        if not lo <= v <= hi:
            raise ValueError("lease filter: %s = %d does not fit" % (name, v))
        f.fields |= bit
        setattr(f, name, v)
    if unattributed:
        f.fields |= SEL_UNATTRIBUTED
    return f


class StreamOutlook(C.Structure):
    """ydc_stream_outlook."""
    _fields_ = [("eligible", C.c_uint32), ("free_servants", C.c_uint32), ("grants_available", C.c_uint64),
                ("running_tasks", C.c_uint64), ("max_tasks", C.c_uint64), ("capacity_available", C.c_uint64),
                ("waiting", C.c_uint32), ("waiting_rows", C.c_uint32), ("leases", C.c_uint32),
                ("zombies", C.c_uint32)]


# numpy view of ydc_stream_outlook (56 bytes)
OUTLOOK_DTYPE = np.dtype([("eligible", "<u4"), ("free_servants", "<u4"), ("grants_available", "<u8"),
                          ("running_tasks", "<u8"), ("max_tasks", "<u8"), ("capacity_available", "<u8"),
                          ("waiting", "<u4"), ("waiting_rows", "<u4"), ("leases", "<u4"), ("zombies", "<u4")])


# numpy view of ydc_book_hit (32 bytes)
HIT_DTYPE = np.dtype([("pos", "<u4"), ("count", "<u4"), ("servant_idx", "<u4"), ("reserved", "<u4"),
                      ("task_grant_id", "<u8"), ("servant_task_id", "<u8")])


# numpy view of ydc_requestor_load (24 bytes)
REQUESTOR_DTYPE = np.dtype([("requestor_ip", "<u4"), ("leases", "<u4"), ("zombies", "<u4"), ("prefetch_leases", "<u4"),
                            ("waiting", "<u4"), ("waiting_rows", "<u4")])


class FairResult(C.Structure):
    """ydc_fair_result (64 bytes)."""
    _fields_ = ([(k, C.c_uint32) for k in ("level", "cap_default_effective", "n_askers", "n_override_askers")] +
                [(k, C.c_uint64) for k in ("pool", "held_total", "held_others", "asked_rows", "capacity_now")] +
                [(k, C.c_uint32) for k in ("tick_no", "mode")])


class DepartCount(C.Structure):
    """ydc_depart_count (20 bytes)."""
    _fields_ = [(k, C.c_uint32) for k in ("requestor_ip", "leases", "zombies", "waiting", "waiting_rows")]


# numpy view of ydc_depart_count
DEPART_DTYPE = np.dtype([(k, "<u4") for k, _ in DepartCount._fields_])


class UsageRow(C.Structure):
    """ydc_usage_row (48 bytes)."""
    _fields_ = ([("requestor_ip", C.c_uint32), ("pad", C.c_uint32)] +
                [(k, C.c_uint64) for k in ("slot_time", "zombie_time", "prefetch_time", "wait_time", "wait_row_time")])


class UsageTotals(C.Structure):
    """ydc_usage_totals."""
    _fields_ = ([(k, C.c_uint64) for k in ("unattributed_time", "quanta", "ticks")] +
                [(k, C.c_uint32) for k in ("n_keys", "slots")])


# numpy view of ydc_usage_row
USAGE_DTYPE = np.dtype([(k, "<u4" if t is C.c_uint32 else "<u8") for k, t in UsageRow._fields_])
USAGE_COLUMNS = ("slot_time", "zombie_time", "prefetch_time", "wait_time", "wait_row_time")
USAGE_RESET = 1  # YDC_USAGE_RESET


# numpy view of ydc_servant_row (32 bytes)
ROW_DTYPE = np.dtype([("version", "<u4"), ("num_processors", "<u4"), ("current_load", "<u4"),
                      ("max_tasks", "<u4"), ("flags", "<u4"), ("ip_id", "<u4"), ("env_mask", "<u8")])


class ServantRow(C.Structure):
    _fields_ = [("version", C.c_uint32), ("num_processors", C.c_uint32),
                ("current_load", C.c_uint32), ("max_tasks", C.c_uint32), ("flags", C.c_uint32),
                ("ip_id", C.c_uint32), ("env_mask", C.c_uint64)]


class TaskSoA(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("env_id", "min_version", "requestor_ip")]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in (
        "n_tasks", "n_servants", "n_classes", "n_slots", "key_bits", "radix_passes", "n_chunks",
        "rounds", "chunk_sims", "granted", "timeouts", "env_not_found", "shard_sort_batches",
        "shard_sort_misses", "small_batch", "zone_rows", "tick_resident_calls", "tick_launched_calls",
        "pipeline_batches")] + [
            ("stage_ms", C.c_float * 16)] + [(k, C.c_uint32) for k in (
                "leases_expired", "leases_swept", "leases_freed", "renewals_refused")]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "stage_ms"}
        d["stage_ms"] = {name: float(self.stage_ms[i]) for i, name in enumerate(STAGES)}
        return d


class StreamCaps(C.Structure):
    """ydc_stream_caps: the bounds of an open stream, in the header's field order."""
    _fields_ = [(k, C.c_uint32) for k in (
        "max_updates", "max_releases", "max_tasks", "max_rows", "max_waiting", "max_leases",
        "max_renewals", "max_frees", "max_reports", "max_report_ids")]


_lib = None


class YdcError(RuntimeError):
    pass


def lib():
    """Loads libydc.so or raises (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YdcError("%s is missing: build it with `make lib` (hipcc --offload-arch=gfx950); "
                           "this package has no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.ydc_strerror.restype = C.c_char_p
        L.ydc_strerror.argtypes = [C.c_int]
        L.ydc_last_error.restype = C.c_char_p
        L.ydc_last_error.argtypes = [C.c_void_p]
        L.ydc_abi_version.restype = C.c_uint32
        L.ydc_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                 C.POINTER(C.c_void_p)]
        L.ydc_destroy.argtypes = [C.c_void_p]
        L.ydc_upload_servants.argtypes = [C.c_void_p, C.POINTER(ServantSoA), C.c_uint32]
        L.ydc_update_servants.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ServantRow),
                                          C.c_uint32]
        L.ydc_update_servants_wide.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ServantRow),
                                               C.c_void_p, C.c_uint32, C.c_uint32]
        L.ydc_set_host_aliases.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_remove_servants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_release_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_release_slots_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_set_running.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_get_running.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_dispatch.argtypes = [C.c_void_p, C.POINTER(TaskSoA), C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p]
        L.ydc_dispatch_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(TaskSoA),
                                        C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ydc_dispatch_device.argtypes = L.ydc_dispatch.argtypes
        L.ydc_dispatch_device_async.argtypes = L.ydc_dispatch.argtypes
        L.ydc_dispatch_wait.argtypes = [C.c_void_p]
        L.ydc_synchronize.argtypes = [C.c_void_p]
        L.ydc_stream_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.ydc_stream_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.c_uint32, C.POINTER(TaskSoA), C.c_uint32, C.c_void_p]
        L.ydc_stream_tick_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(TaskSoA),
                                           C.c_uint32, C.c_void_p]
        L.ydc_stream_buffers_get.argtypes = [C.c_void_p, C.c_void_p]
        L.ydc_stream_end.argtypes = [C.c_void_p]
        L.ydc_stream_begin_waiting.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.ydc_stream_tick_waiting.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(TaskSoA),
                                              C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32)]
        L.ydc_stream_waiting_take.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.ydc_stream_begin_leased.argtypes = [C.c_void_p] + [C.c_uint32] * 8
        L.ydc_stream_tick_leased.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,  # heartbeats
            C.c_void_p, C.c_uint32,                                                  # releases by servant
            C.c_void_p, C.c_void_p, C.c_uint32,                                      # renewals
            C.c_void_p, C.c_uint32,                                                  # frees by id
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,                          # reports (CSR)
            C.POINTER(TaskSoA), C.c_void_p, C.c_uint32, C.c_int64,                   # requests, clock
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.ydc_stream_begin_waiting_leased.argtypes = [C.c_void_p] + [C.c_uint32] * 9
        L.ydc_stream_tick_waiting_leased.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,  # heartbeats
            C.c_void_p, C.c_uint32,                                                  # releases by servant
            C.c_void_p, C.c_void_p, C.c_uint32,                                      # renewals
            C.c_void_p, C.c_uint32,                                                  # frees by id
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,                          # reports (CSR)
            C.POINTER(TaskSoA), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64,  # requests, clock
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),   # as a leased tick
            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]  # resolved list
        L.ydc_stream_begin_rpc.argtypes = [C.c_void_p] + [C.c_uint32] * 10
        L.ydc_stream_tick_rpc.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,  # heartbeats
            C.c_void_p, C.c_uint32,                                                  # releases by servant
            C.c_void_p, C.c_void_p, C.c_uint32,                                      # renewals
            C.c_void_p, C.c_uint32,                                                  # frees by id
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,                          # reports (CSR)
            C.POINTER(TaskSoA), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,  # requests
            C.c_uint32, C.c_int64,                                                   # n_req, clock
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,                          # status, count, rows
            C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),                           # as a leased tick
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,  # resolved list, its grants
            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.ydc_stream_leases_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.POINTER(C.c_uint32)]
        L.ydc_stream_caps_get.argtypes = [C.c_void_p, C.POINTER(StreamCaps)]
        L.ydc_stream_reserve.argtypes = [C.c_void_p, C.POINTER(StreamCaps)]
        L.ydc_stream_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ydc_stream_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(StreamCaps)]
        L.ydc_stream_delta_base.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ydc_stream_delta.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ydc_stream_delta_apply.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.ydc_stream_delta_stop.argtypes = [C.c_void_p]
        L.ydc_stream_delta_inspect.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ydc_stream_inspect_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.ydc_stream_delta_apply_inspected.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.ydc_stream_alive_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_alive_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_alive_removed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ydc_stream_alive_get.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.ydc_debug_alive.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ydc_debug_pipeline.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ydc_stream_inspect_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_inspect_load.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint32]
        L.ydc_stream_inspect_servants.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_void_p]
        L.ydc_stream_inspect_tasks.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p]
        L.ydc_stream_outlook_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.ydc_stream_inspect_waiting.argtypes = [C.c_void_p] + [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p]
        L.ydc_stream_inspect_select.argtypes = [C.c_void_p, C.POINTER(LeaseFilter)] + [C.c_void_p] * 8 + [
            C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.ydc_stream_inspect_count.argtypes = [C.c_void_p, C.POINTER(LeaseFilter), C.c_uint32, C.c_void_p]
        L.ydc_stream_requestor_find.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.ydc_stream_requestor_get.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32)]
        L.ydc_admit_clip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_void_p]
        L.ydc_stream_withdraw_begin.argtypes = [C.c_void_p, C.c_uint32]
        L.ydc_stream_withdraw_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_withdraw_result.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ydc_stream_quota_begin.argtypes = [C.c_void_p, C.c_uint32]
        L.ydc_stream_quota_set.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_quota_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.ydc_stream_quota_fair.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.ydc_stream_quota_fair_result.argtypes = [C.c_void_p, C.POINTER(FairResult)]
        L.ydc_fair_level.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64,
                                     C.POINTER(C.c_uint32)]
        L.ydc_stream_depart_begin.argtypes = [C.c_void_p, C.c_uint32]
        L.ydc_stream_depart_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_depart_result.argtypes = [C.c_void_p, C.POINTER(DepartCount), C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.ydc_stream_usage_begin.argtypes = [C.c_void_p, C.c_int64, C.c_uint32]
        L.ydc_stream_usage_get.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_usage_find.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.ydc_stream_usage_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.ydc_usage_quanta.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64)]
        L.ydc_stream_book_begin.argtypes = [C.c_void_p, C.c_uint32]
        L.ydc_stream_book_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.ydc_stream_book_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.POINTER(C.c_uint32)]
        L.ydc_stream_book_find.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.ydc_stream_book_distinct.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint32, C.POINTER(C.c_uint32),
                                                                                  C.POINTER(C.c_uint32)]
        L.ydc_group_unique_id.argtypes = [C.c_void_p]
        L.ydc_group_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ydc_group_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.ydc_group_destroy.argtypes = [C.c_void_p]
        L.ydc_group_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ydc_group_ipc_export.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ydc_group_init_ipc.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ydc_group_transport.argtypes = [C.c_void_p]
        L.ydc_dispatch_sharded.argtypes = L.ydc_dispatch.argtypes
        L.ydc_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.ydc_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.ydc_kernel_profile.argtypes = [C.c_void_p]
        L.ydc_kernel_profile.restype = C.c_char_p
        L.ydc_device_count.restype = C.c_int
        L.ydc_device_malloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.ydc_device_free.argtypes = [C.c_void_p]
        L.ydc_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.ydc_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.ydc_host_register.argtypes = [C.c_void_p, C.c_size_t]
        L.ydc_host_unregister.argtypes = [C.c_void_p]
        L.ydc_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.ydc_host_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, DeviceArray):
        return a.ptr
    if isinstance(a, int):
        return a
    return a.data_ptr()  # anything torch-like


# The library reads ONE developer variable, YDC_TUNE="key=value,...". The tests and measurement
# scripts of this repository name their switches YDC_<KEY>=<value>: compose_tune() folds those
# into YDC_TUNE right before a context is created (and takes out again what it folded in last
# time, so that a switch a test has dropped is gone). Not an interface of the package.
_TUNE_KEYS = ("DEBUG_SIM", "CHUNK_SIZE", "TARGET_CHUNKS", "FUSED_CLASS", "OWN_GUESS", "PAIR", "RING_TOTAL",
              "GROUP_WALK", "WALK_PACKED", "ZONE_GUESS", "ZONE_LEAD", "ZONE_TRAIL", "ZONE_MAX_CHUNKS",
              "PACKED_CLASS", "SHARD_SORT", "BINSORT", "FUSE_PASSES", "WARM_UP",
              "HAND_TRIES", "LANES", "CP_EVERY", "WALK_PARK", "WIDE", "WIDE_LISTS", "GROUP_BINSORT",
              "BINSORT_VERIFY", "BINSORT_MAX_SLOTS", "BIN_THREADS", "SHARD_MARGIN",
              "ROUNDS_PER_CHECK", "WALK_AFTER", "OUTCOME_STORE", "STREAM_GRAPH", "COMMIT_SWAP", "RELEASE_COUNTED", "SMALL_BATCH", "RESIDENT", "RESIDENT_IDLE_MS", "PACKED_TICK", "IPC_SLOT_WORDS", "IPC_TIMEOUT_MS", "IPC_COARSE",
              "REQUESTOR_COMBINE")
_tune_injected = ""


def compose_tune():
    """The folded YDC_<KEY> switches go FIRST: the library takes the first match of a key, so a
    test's switch wins over the same key in an inherited YDC_TUNE."""
    global _tune_injected
    cur = os.environ.get("YDC_TUNE", "")
    if _tune_injected and cur.startswith(_tune_injected):
        cur = cur[len(_tune_injected):].lstrip(",")
    mine = ",".join("%s=%s" % (k.lower(), os.environ["YDC_" + k]) for k in _TUNE_KEYS
                    if "YDC_" + k in os.environ)
    _tune_injected = mine
    both = ",".join(x for x in (mine, cur) if x)
    if both:
        os.environ["YDC_TUNE"] = both
    else:
        os.environ.pop("YDC_TUNE", None)


def admit_clip(requestor_ip, n_immediate, n_prefetch, load, cap):
    """The admission arithmetic (ydc_admit_clip; no context, no device): the tick's rows in arrival
    order, load a REQUESTOR_DTYPE array with load[i] for requestor_ip[i], cap the grants a requestor
    may have outstanding. n_prefetch: None means zeros. -> (out_immediate, out_prefetch), uint32."""
    ips = np.ascontiguousarray(requestor_ip, dtype=np.uint32)
    imm = np.ascontiguousarray(n_immediate, dtype=np.uint32)
    pre = None if n_prefetch is None else np.ascontiguousarray(n_prefetch, dtype=np.uint32)
    ld = np.ascontiguousarray(load, dtype=REQUESTOR_DTYPE)
    assert ips.ndim == 1 and imm.shape == ips.shape and ld.shape == ips.shape and (pre is None or pre.shape == ips.shape)
    out_imm, out_pre = np.zeros(len(ips), np.uint32), np.zeros(len(ips), np.uint32)
    rc = lib().ydc_admit_clip(_ptr(ips), _ptr(imm), _ptr(pre), len(ips), _ptr(ld), int(cap), _ptr(out_imm), _ptr(out_pre))
    if rc:
        raise YdcError("ydc_admit_clip: %s (a load with unknown lease columns?)" % lib().ydc_strerror(rc).decode())
    return out_imm, out_pre


def fair_level(held, asked, fixed_cap=None, others=0, pool=0):
    """The fair-share level (ydc_fair_level; no context, no device): requestor i holds held[i] and asks
    asked[i]; fixed_cap[i] its override, QUOTA_UNLIMITED (or fixed_cap None) for a requestor inside the
    fair share; others: what everybody else holds; pool: what may be held in all. -> the level,
    QUOTA_UNLIMITED when all demand fits."""
    h = np.ascontiguousarray(held, dtype=np.uint32)
    a = np.ascontiguousarray(asked, dtype=np.uint32)
    f = None if fixed_cap is None else np.ascontiguousarray(fixed_cap, dtype=np.uint32)
    assert h.ndim == 1 and a.shape == h.shape and (f is None or f.shape == h.shape)
    out = C.c_uint32(0)
    rc = lib().ydc_fair_level(_ptr(h), _ptr(a), _ptr(f), len(h), int(others), int(pool), C.byref(out))
    if rc:
        raise YdcError("ydc_fair_level: %s" % lib().ydc_strerror(rc).decode())
    return int(out.value)


def usage_quanta(last, now, quantum):
    """The quanta a tick at `now` charges after one at `last` (ydc_usage_quanta; no context, no device):
    floor(now / quantum) - floor(last / quantum) modulo 2^64."""
    out = C.c_uint64(0)
    rc = lib().ydc_usage_quanta(int(last), int(now), int(quantum), C.byref(out))
    if rc:
        raise YdcError("ydc_usage_quanta: %s" % lib().ydc_strerror(rc).decode())
    return int(out.value)


def device_count():
    """GPUs visible to the library's HIP runtime (0 when the library is missing)."""
    try:
        return int(lib().ydc_device_count())
    except (YdcError, OSError):
        return 0


def pinned_empty(n, dtype):
    """A numpy array in page-locked host memory the device can address (ydc_host_alloc): request
    columns and result arrays of this kind go through ydc_dispatch without any staging copy.
    The memory is freed when the array (and every view of it) is gone."""
    dt = np.dtype(dtype)
    p = C.c_void_p()
    rc = lib().ydc_host_alloc(int(n) * dt.itemsize, C.byref(p))
    if rc:
        raise YdcError("ydc_host_alloc: %s (%s)" % (lib().ydc_strerror(rc).decode(),
                                                    lib().ydc_last_error(None).decode()))
    buf = (C.c_char * max(1, int(n) * dt.itemsize)).from_address(p.value)
    import weakref
    weakref.finalize(buf, lib().ydc_host_free, p.value)  # numpy keeps `buf` alive through .base
    return np.frombuffer(buf, dtype=dt, count=int(n))


def host_register(a):
    """Page-locks the memory of a contiguous numpy array in place (ydc_host_register); the array
    must stay alive and unmoved until host_unregister(a)."""
    assert a.flags.c_contiguous
    rc = lib().ydc_host_register(a.ctypes.data, a.nbytes)
    if rc:
        raise YdcError("ydc_host_register: %s (%s)" % (lib().ydc_strerror(rc).decode(),
                                                       lib().ydc_last_error(None).decode()))


def host_unregister(a):
    rc = lib().ydc_host_unregister(a.ctypes.data)
    if rc:
        raise YdcError("ydc_host_unregister: %s" % lib().ydc_strerror(rc).decode())


def group_unique_id():
    """128-byte id for Context.group_init (ncclGetUniqueId); call on one rank, hand to all."""
    buf = C.create_string_buffer(128)
    rc = lib().ydc_group_unique_id(buf)
    if rc:
        raise YdcError("ydc_group_unique_id: %s (%s)" % (lib().ydc_strerror(rc).decode(),
                                                         lib().ydc_last_error(None).decode()))
    return buf.raw


def group_init_local(contexts):
    """Makes the given contexts (one process, one device) the ranks of a group that exchanges
    through device copies; each rank's dispatch_sharded must then run in its own thread."""
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = lib().ydc_group_init_local(arr, len(contexts))
    if rc:
        raise YdcError("ydc_group_init_local: %s" % lib().ydc_strerror(rc).decode())


class DeviceArray:
    """A typed buffer in HBM owned by the caller (hipMalloc through the C-ABI)."""

    def __init__(self, n, dtype, device=0):
        self.n, self.dtype, self.device = int(n), np.dtype(dtype), device
        p = C.c_void_p()
        rc = lib().ydc_device_malloc(device, self.n * self.dtype.itemsize, C.byref(p))
        if rc:
            raise YdcError("ydc_device_malloc: %s (%s)" % (
                lib().ydc_strerror(rc).decode(), lib().ydc_last_error(None).decode()))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        d = cls(a.size, a.dtype, device)
        if a.size and lib().ydc_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes):
            raise YdcError("ydc_memcpy_h2d failed")
        return d

    def numpy(self):
        out = np.empty(self.n, self.dtype)
        if self.n and lib().ydc_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes):
            raise YdcError("ydc_memcpy_d2h failed")
        return out

    def numel(self):
        return self.n

    def free(self):
        if self.ptr:
            lib().ydc_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _depart_count(v, name):
    """A capacity of the departure calls: a whole number that fits uint32 (no silent wrap)."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__))
    if not 0 <= int(v) < 1 << 32:
        raise ValueError("%s %d does not fit uint32" % (name, int(v)))
    return int(v)


def _depart_keys(requestors):
    """The staged requestors as a contiguous uint32 column; anything that is not a flat sequence of whole
    numbers in [0, 2^32) is refused here (numpy would wrap or truncate it)."""
    a = np.asarray(requestors)
    if a.ndim != 1:
        raise TypeError("requestors must be a flat sequence of requestor_ip ids")
    if a.size == 0:
        return np.empty(0, np.uint32)
    if a.dtype.kind not in "iu":
        raise TypeError("requestors must be whole numbers (requestor_ip ids), not %s" % a.dtype)
    if int(a.min()) < 0 or int(a.max()) >= 1 << 32:
        raise ValueError("a requestor_ip id does not fit uint32")
    return np.ascontiguousarray(a, dtype=np.uint32)


class Context:
    """One ydc_context: a resident servant registry on one GPU + batch dispatch."""

    def __init__(self, device=0, max_servants=0, max_tasks=0, max_slots=0, stream=None):
        h = C.c_void_p()
        compose_tune()
        rc = lib().ydc_create(device, max_servants, max_tasks, max_slots, stream, C.byref(h))
        if rc:
            raise YdcError("ydc_create: %s (%s)" % (lib().ydc_strerror(rc).decode(),
                                                    lib().ydc_last_error(None).decode()))
        self._h = h
        self.n_servants = 0
        self._stream_caps = (0, 0, 0)
        self._max_waiting = 0
        self._max_rows = 0
        self._alive = False
        self._alive_removals = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().ydc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise YdcError("%s: %s (%s)" % (what, lib().ydc_strerror(rc).decode(),
                                            lib().ydc_last_error(self._h).decode()))

    def upload_servants(self, cols):
        """cols: dict of numpy columns named like ydc_servant_soa (see pack.to_abi_columns).
        env_mask: (n,) for up to 64 interned digests, or (n, env_words)."""
        keep = {}
        soa = ServantSoA()
        for k, dt in (("version", np.uint32), ("num_processors", np.uint32),
                      ("current_load", np.uint32), ("max_tasks", np.uint32),
                      ("running_tasks", np.uint32), ("flags", np.uint32),
                      ("env_mask", np.uint64), ("ip_id", np.uint32)):
            keep[k] = np.ascontiguousarray(cols[k], dtype=dt)
            setattr(soa, k, keep[k].ctypes.data)
        n = len(keep["version"])
        soa.env_words = keep["env_mask"].shape[1] if keep["env_mask"].ndim == 2 else 1
        self._check(lib().ydc_upload_servants(self._h, C.byref(soa), n), "ydc_upload_servants")
        self.n_servants = n

    def update_servants(self, idx, rows, env_masks=None):
        """rows: dicts named like ydc_servant_row. env_masks: optional (len(rows), env_words)
        uint64 array for registries with more than 64 interned digests (rows' env_mask is
        ignored then)."""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        arr = (ServantRow * len(rows))()
        for i, r in enumerate(rows):
            for k in ("version", "num_processors", "current_load", "max_tasks", "flags", "ip_id",
                      "env_mask"):
                setattr(arr[i], k, int(r.get(k, 0)) if isinstance(r, dict) else int(r[k]))
        if env_masks is None:
            self._check(lib().ydc_update_servants(self._h, idx.ctypes.data, arr, len(rows)),
                        "ydc_update_servants")
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(rows), -1)
            self._check(lib().ydc_update_servants_wide(self._h, idx.ctypes.data, arr,
                                                       em.ctypes.data, em.shape[1], len(rows)),
                        "ydc_update_servants_wide")
        if len(idx):
            self.n_servants = max(self.n_servants, int(idx.max()) + 1)

    def set_host_aliases(self, ip_id, servant_idx):
        """Further (host id, servant row) entries of the requestor-address lookup table."""
        a = np.ascontiguousarray(ip_id, dtype=np.uint32)
        b = np.ascontiguousarray(servant_idx, dtype=np.uint32)
        assert len(a) == len(b)
        self._check(lib().ydc_set_host_aliases(self._h, a.ctypes.data, b.ctypes.data, len(a)),
                    "ydc_set_host_aliases")

    def remove_servants(self, idx):
        """Servant expiry: rows idx (ascending) leave, the rest keeps its order."""
        a = np.ascontiguousarray(idx, dtype=np.uint32)
        self._check(lib().ydc_remove_servants(self._h, a.ctypes.data, len(a)),
                    "ydc_remove_servants")
        self.n_servants -= len(a)

    def release_slots(self, servant_idx):
        a = np.ascontiguousarray(servant_idx, dtype=np.uint32)
        self._check(lib().ydc_release_slots(self._h, a.ctypes.data, len(a)), "ydc_release_slots")

    def release_slots_device(self, d_servant_idx):
        """Indexes already in device memory (a DeviceArray / tensor, e.g. a batch's placement output):
        entries that are no servant index are skipped; no staging copy."""
        self._check(lib().ydc_release_slots_device(self._h, _ptr(d_servant_idx), int(d_servant_idx.numel())),
                    "ydc_release_slots_device")

    def set_running(self, running):
        a = np.ascontiguousarray(running, dtype=np.uint32)
        self._check(lib().ydc_set_running(self._h, a.ctypes.data, len(a)), "ydc_set_running")

    def get_running(self):
        out = np.empty(self.n_servants, np.uint32)
        self._check(lib().ydc_get_running(self._h, out.ctypes.data, len(out)), "ydc_get_running")
        return out

    def dispatch(self, tasks, commit=False, want_util=True, want_running=True, out_idx=None):
        """Host numpy columns in, numpy out: (servant_idx, utilization|None, running_after|None).
        out_idx: a uint32 array of the batch's length to write the placement into (a caller that
        dispatches batch after batch reuses its buffer; a fresh 400 KB array per call is page
        faults, not dispatch)."""
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = out_idx if out_idx is not None else np.empty(n, np.uint32)
        assert out.dtype == np.uint32 and out.size == n and out.flags.c_contiguous
        util = np.empty(n, np.float64) if want_util else None
        run = np.empty(self.n_servants, np.uint32) if want_running else None
        self._check(lib().ydc_dispatch(self._h, C.byref(soa), n, DISPATCH_COMMIT if commit else 0,
                                       _ptr(out), _ptr(util), _ptr(run)), "ydc_dispatch")
        return out, util, run

    def dispatch_tick(self, tasks, upd_idx=(), upd_rows=None, release_idx=(), env_masks=None,
                      commit=True, want_util=False):
        """One scheduler turn (ydc_dispatch_tick): heartbeat rows (structured array of ROW_DTYPE),
        released grants (servant index each), then the requests. Returns (servant_idx, util|None)."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows if upd_rows is not None else np.zeros(0, ROW_DTYPE),
                                  dtype=ROW_DTYPE)
        assert len(ur) == len(ui)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = np.empty(n, np.uint32)
        util = np.empty(n, np.float64) if want_util else None
        em = None
        if env_masks is not None:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64)
            em = em.reshape(len(ui), em.shape[-1] if em.ndim == 2 else max(1, em.size // max(1, len(ui))))
        self._check(lib().ydc_dispatch_tick(self._h, ui.ctypes.data, ur.ctypes.data,
                                            em.ctypes.data if em is not None else None,
                                            em.shape[1] if em is not None else 1, len(ui),
                                            rel.ctypes.data, len(rel), C.byref(soa), n,
                                            DISPATCH_COMMIT if commit else 0, out.ctypes.data,
                                            _ptr(util)), "ydc_dispatch_tick")
        return out, util

    def dispatch_device(self, d_env, d_minv, d_ip, d_out_idx=None, d_out_util=None,
                        d_out_running=None, commit=False):
        """Device buffers (torch tensors): task columns and outputs already in HBM."""
        soa = TaskSoA(_ptr(d_env), _ptr(d_minv), _ptr(d_ip))
        n = int(d_env.numel())
        self._check(lib().ydc_dispatch_device(self._h, C.byref(soa), n,
                                              DISPATCH_COMMIT if commit else 0, _ptr(d_out_idx),
                                              _ptr(d_out_util), _ptr(d_out_running)),
                    "ydc_dispatch_device")

    def dispatch_device_async(self, d_env, d_minv, d_ip, d_out_idx=None, d_out_util=None,
                              d_out_running=None, commit=False):
        """Pipelined dispatch_device: enqueues the batch and returns; dispatch_wait() waits for
        the oldest outstanding batch (at most two may be outstanding)."""
        soa = TaskSoA(_ptr(d_env), _ptr(d_minv), _ptr(d_ip))
        n = int(d_env.numel())
        self._check(lib().ydc_dispatch_device_async(self._h, C.byref(soa), n,
                                                    DISPATCH_COMMIT if commit else 0,
                                                    _ptr(d_out_idx), _ptr(d_out_util),
                                                    _ptr(d_out_running)),
                    "ydc_dispatch_device_async")

    def dispatch_wait(self):
        self._check(lib().ydc_dispatch_wait(self._h), "ydc_dispatch_wait")

    def synchronize(self):
        self._check(lib().ydc_synchronize(self._h), "ydc_synchronize")

    def debug_pipeline(self):
        """Tests and tools: (batches placed so far, pipelined batches that were enqueued on the second
        device lane, batches dispatch_wait had to place again)."""
        b, s, m = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(lib().ydc_debug_pipeline(self._h, C.byref(b), C.byref(s), C.byref(m)), "ydc_debug_pipeline")
        return int(b.value), int(s.value), int(m.value)

    # -- multi-GPU group ---------------------------------------------------------------
    def group_init(self, unique_id, rank, n_ranks):
        """Collective (like ncclCommInitRank). unique_id: the 128 bytes of group_unique_id()."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(lib().ydc_group_init(self._h, buf, rank, n_ranks), "ydc_group_init")

    def group_size(self):
        """(ranks, is_rccl): for an RCCL group the count is ncclCommCount of the communicator."""
        n, r = C.c_int(0), C.c_int(0)
        self._check(lib().ydc_group_size(self._h, C.byref(n), C.byref(r)), "ydc_group_size")
        return n.value, bool(r.value)

    def group_ipc_export(self, rank, n_ranks):
        """This rank's mailbox handle (IPC_HANDLE_BYTES bytes) for the RCCL-free inter-process
        transport; the launcher all-gathers the handles and every rank calls group_init_ipc."""
        buf = C.create_string_buffer(IPC_HANDLE_BYTES)
        self._check(lib().ydc_group_ipc_export(self._h, rank, n_ranks, buf), "ydc_group_ipc_export")
        return buf.raw

    def group_init_ipc(self, handles, rank, n_ranks, transport=TRANSPORT_IPC_DEVICE):
        """handles: the n_ranks exported handles in rank order. Every rank passes the same
        transport (TRANSPORT_IPC_DEVICE: HIP IPC device memory; TRANSPORT_IPC_HOST: shared host
        segment). Raises if a peer's mailbox cannot be mapped — the export stays, so the
        launcher may agree on the other flavour and call again."""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == n_ranks * IPC_HANDLE_BYTES
        buf = C.create_string_buffer(blob, len(blob))
        self._check(lib().ydc_group_init_ipc(self._h, buf, rank, n_ranks, transport),
                    "ydc_group_init_ipc")

    def group_transport(self):
        """TRANSPORT_* of the group this context is a rank of."""
        return int(lib().ydc_group_transport(self._h))

    def group_destroy(self):
        self._check(lib().ydc_group_destroy(self._h), "ydc_group_destroy")

    def dispatch_sharded(self, d_env, d_minv, d_ip, d_out_idx=None, d_out_util=None,
                         d_out_running=None, commit=False):
        """Collective: this rank's slice of the global batch (device buffers)."""
        soa = TaskSoA(_ptr(d_env), _ptr(d_minv), _ptr(d_ip))
        n = int(d_env.numel())
        self._check(lib().ydc_dispatch_sharded(self._h, C.byref(soa), n,
                                               DISPATCH_COMMIT if commit else 0, _ptr(d_out_idx),
                                               _ptr(d_out_util), _ptr(d_out_running)),
                    "ydc_dispatch_sharded")

    # -- streaming mode: one captured step per tick ---------------------------------
    def stream_begin(self, max_updates, max_releases, max_tasks, max_waiting=0):
        """max_waiting > 0: waiting mode (ydc_stream_begin_waiting) — requests that find no free
        servant wait in a queue on the device until granted, EnvironmentNotFound or their deadline
        (stream_tick_waiting); max_waiting bounds the queue plus a tick's new requests."""
        if max_waiting:
            self._check(lib().ydc_stream_begin_waiting(self._h, max_updates, max_releases, max_tasks,
                                                       max_waiting), "ydc_stream_begin_waiting")
        else:
            self._check(lib().ydc_stream_begin(self._h, max_updates, max_releases, max_tasks),
                        "ydc_stream_begin")
        self._stream_caps = (int(max_updates), int(max_releases), int(max_tasks))
        self._alive = False
        self._max_waiting = int(max_waiting)

    def stream_tick_waiting(self, upd_idx, upd_rows, release_idx, tasks, deadlines, tags, now,
                            env_masks=None):
        """One tick of a context begun with max_waiting > 0 (ydc_stream_tick_waiting).
        deadlines: int64 per request, tags: uint64 per request (echoed back), now: int64 clock of
        the tick (never smaller than the previous tick's). Returns (out, resolved_tags,
        resolved_idx, n_waiting): out[i] is the servant index, IDX_TIMEOUT, IDX_ENV_NOT_FOUND or
        IDX_WAITING of request i; the resolved list holds the queued requests answered in this
        tick, in queue order; n_waiting is the size of the queue afterwards."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows, dtype=ROW_DTYPE)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        dl = np.ascontiguousarray(deadlines, dtype=np.int64)
        tg = np.ascontiguousarray(tags, dtype=np.uint64)
        assert len(dl) == n and len(tg) == n
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = np.empty(n, np.uint32)
        cap = max(self._max_waiting, 1)
        res_tags = np.empty(cap, np.uint64)
        res_idx = np.empty(cap, np.uint32)
        n_res, n_wait = C.c_uint32(0), C.c_uint32(0)
        if env_masks is None:
            em, words = None, 1
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(ui), -1)
            words = em.shape[1]
        self._check(lib().ydc_stream_tick_waiting(
            self._h, ui.ctypes.data, ur.ctypes.data, None if em is None else em.ctypes.data, words,
            len(ui), rel.ctypes.data, len(rel), C.byref(soa), dl.ctypes.data, tg.ctypes.data, n,
            int(now), out.ctypes.data, res_tags.ctypes.data, res_idx.ctypes.data, C.byref(n_res),
            C.byref(n_wait)), "ydc_stream_tick_waiting")
        k = n_res.value
        return out, res_tags[:k].copy(), res_idx[:k].copy(), int(n_wait.value)

    def stream_begin_leased(self, max_updates, max_releases, max_tasks, max_leases, max_renewals,
                            max_frees, max_reports, max_report_ids):
        """Leased mode (ydc_stream_begin_leased): the context remembers every grant in a lease table
        on the device (task id, servant, expiry, zombie flag); ticks go through stream_tick_leased."""
        self._check(lib().ydc_stream_begin_leased(self._h, max_updates, max_releases, max_tasks, max_leases,
                                                  max_renewals, max_frees, max_reports, max_report_ids),
                    "ydc_stream_begin_leased")
        self._stream_caps = (int(max_updates), int(max_releases), int(max_tasks))
        self._alive = False
        self._max_waiting = 0
        self._max_leases = int(max_leases)

    def stream_tick_leased(self, upd_idx, upd_rows, release_idx, renew_ids, renew_expires_at, free_ids,
                           report_servants, report_off, report_ids, tasks, lease_expires_at, now,
                           env_masks=None):
        """One tick of a context begun with stream_begin_leased (ydc_stream_tick_leased): heartbeats,
        renewals (uint64 ids, int64 new expiries), frees by id, releases by servant index, expiry at
        clock `now`, servant reports in CSR form (report_off has len(report_servants) + 1 entries),
        then the requests with their per-request lease_expires_at. Returns (out, task_ids, renewed,
        report_unknown, n_leases): out[i] as stream_tick, task_ids[i] the grant's id (only where
        out[i] is a servant), renewed[i] / report_unknown[k] as uint8 flags, n_leases = |L| afterwards."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows, dtype=ROW_DTYPE)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        rid = np.ascontiguousarray(renew_ids, dtype=np.uint64)
        rex = np.ascontiguousarray(renew_expires_at, dtype=np.int64)
        fid = np.ascontiguousarray(free_ids, dtype=np.uint64)
        rs = np.ascontiguousarray(report_servants, dtype=np.uint32)
        ro = np.ascontiguousarray(report_off, dtype=np.uint32)
        ri = np.ascontiguousarray(report_ids, dtype=np.uint64)
        assert len(rid) == len(rex) and (len(rs) == 0 or len(ro) == len(rs) + 1)
        assert len(rs) == 0 or int(ro[-1]) == len(ri)
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        lex = np.ascontiguousarray(lease_expires_at, dtype=np.int64)
        assert len(lex) == n
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = np.empty(n, np.uint32)
        ids = np.empty(n, np.uint64)
        renewed = np.zeros(len(rid), np.uint8)
        unknown = np.zeros(len(ri), np.uint8)
        n_leases = C.c_uint32(0)
        if env_masks is None:
            em, words = None, 1
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(ui), -1)
            words = em.shape[1]
        self._check(lib().ydc_stream_tick_leased(
            self._h, ui.ctypes.data, ur.ctypes.data, None if em is None else em.ctypes.data, words, len(ui),
            rel.ctypes.data, len(rel), rid.ctypes.data, rex.ctypes.data, len(rid), fid.ctypes.data, len(fid),
            rs.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(rs), C.byref(soa), lex.ctypes.data, n, int(now),
            out.ctypes.data, ids.ctypes.data, renewed.ctypes.data, unknown.ctypes.data, C.byref(n_leases)),
            "ydc_stream_tick_leased")
        self._alive_shrink()
        return out, ids, renewed, unknown, int(n_leases.value)

    def stream_begin_waiting_leased(self, max_updates, max_releases, max_tasks, max_waiting, max_leases,
                                    max_renewals, max_frees, max_reports, max_report_ids):
        """Waiting queue and lease table at once (ydc_stream_begin_waiting_leased): requests that find
        no free servant wait on the device, and every grant, a waiter's included, takes its task id
        and its lease there; ticks go through stream_tick_waiting_leased."""
        self._check(lib().ydc_stream_begin_waiting_leased(
            self._h, max_updates, max_releases, max_tasks, max_waiting, max_leases, max_renewals, max_frees,
            max_reports, max_report_ids), "ydc_stream_begin_waiting_leased")
        self._stream_caps = (int(max_updates), int(max_releases), int(max_tasks))
        self._alive = False
        self._max_waiting = int(max_waiting)
        self._max_leases = int(max_leases)

    def stream_tick_waiting_leased(self, upd_idx, upd_rows, release_idx, renew_ids, renew_expires_at, free_ids,
                                   report_servants, report_off, report_ids, tasks, lease_for, deadlines, tags,
                                   now, env_masks=None):
        """One tick of a context begun with stream_begin_waiting_leased
        (ydc_stream_tick_waiting_leased): the arguments of stream_tick_leased with lease_for (int64
        duration per request; a lease runs from its grant: expires_at = now of the granting tick +
        lease_for) in place of lease_expires_at, plus deadlines and tags as stream_tick_waiting.
        Returns (out, task_ids, renewed, report_unknown, n_leases, resolved_tags, resolved_idx,
        resolved_task_ids, n_waiting): the resolved list holds the queued requests answered in this
        tick in queue order, resolved_task_ids[i] the id of a queued request's grant (only where
        resolved_idx[i] is a servant); ids go to the queue's grants first, then to the new ones."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows, dtype=ROW_DTYPE)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        rid = np.ascontiguousarray(renew_ids, dtype=np.uint64)
        rex = np.ascontiguousarray(renew_expires_at, dtype=np.int64)
        fid = np.ascontiguousarray(free_ids, dtype=np.uint64)
        rs = np.ascontiguousarray(report_servants, dtype=np.uint32)
        ro = np.ascontiguousarray(report_off, dtype=np.uint32)
        ri = np.ascontiguousarray(report_ids, dtype=np.uint64)
        assert len(rid) == len(rex) and (len(rs) == 0 or len(ro) == len(rs) + 1)
        assert len(rs) == 0 or int(ro[-1]) == len(ri)
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        lfor = np.ascontiguousarray(lease_for, dtype=np.int64)
        dl = np.ascontiguousarray(deadlines, dtype=np.int64)
        tg = np.ascontiguousarray(tags, dtype=np.uint64)
        assert len(lfor) == n and len(dl) == n and len(tg) == n
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = np.empty(n, np.uint32)
        ids = np.empty(n, np.uint64)
        renewed = np.zeros(len(rid), np.uint8)
        unknown = np.zeros(len(ri), np.uint8)
        cap = max(self._max_waiting, 1)
        res_tags, res_idx, res_ids = np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint64)
        n_leases, n_res, n_wait = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if env_masks is None:
            em, words = None, 1
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(ui), -1)
            words = em.shape[1]
        self._check(lib().ydc_stream_tick_waiting_leased(
            self._h, ui.ctypes.data, ur.ctypes.data, None if em is None else em.ctypes.data, words, len(ui),
            rel.ctypes.data, len(rel), rid.ctypes.data, rex.ctypes.data, len(rid), fid.ctypes.data, len(fid),
            rs.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(rs), C.byref(soa), lfor.ctypes.data,
            dl.ctypes.data, tg.ctypes.data, n, int(now), out.ctypes.data, ids.ctypes.data, renewed.ctypes.data,
            unknown.ctypes.data, C.byref(n_leases), res_tags.ctypes.data, res_idx.ctypes.data,
            res_ids.ctypes.data, C.byref(n_res), C.byref(n_wait)), "ydc_stream_tick_waiting_leased")
        self._alive_shrink()
        k = n_res.value
        return (out, ids, renewed, unknown, int(n_leases.value), res_tags[:k].copy(), res_idx[:k].copy(),
                res_ids[:k].copy(), int(n_wait.value))

    def stream_begin_rpc(self, max_updates, max_releases, max_requests, max_rows, max_waiting, max_leases,
                         max_renewals, max_frees, max_reports, max_report_ids):
        """One request row per WaitForStartingTask RPC (ydc_stream_begin_rpc): a waiting and leased
        context whose requests ask for n_immediate + n_prefetch grants each; max_rows bounds the
        expanded batch. Ticks go through stream_tick_rpc."""
        self._check(lib().ydc_stream_begin_rpc(
            self._h, max_updates, max_releases, max_requests, max_rows, max_waiting, max_leases, max_renewals,
            max_frees, max_reports, max_report_ids), "ydc_stream_begin_rpc")
        self._stream_caps = (int(max_updates), int(max_releases), int(max_requests))
        self._alive = False
        self._max_waiting = int(max_waiting)
        self._max_leases = int(max_leases)
        self._max_rows = int(max_rows)

    def stream_tick_rpc(self, upd_idx, upd_rows, release_idx, renew_ids, renew_expires_at, free_ids,
                        report_servants, report_off, report_ids, requests, n_immediate, n_prefetch, lease_for,
                        deadlines, tags, now, env_masks=None):
        """One tick of a context begun with stream_begin_rpc (ydc_stream_tick_rpc): the arguments of
        stream_tick_waiting_leased with the two counts per request. Returns a dict: status and
        n_granted per request; servants and task_ids in expanded layout (request i's rows at
        row_off[i], the first n_granted[i] defined); renewed, report_unknown, n_leases; the resolved
        list res_tags, res_status, res_n_granted, res_first with its grants packed in res_servants /
        res_task_ids; n_waiting, n_waiting_rows."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows, dtype=ROW_DTYPE)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        rid = np.ascontiguousarray(renew_ids, dtype=np.uint64)
        rex = np.ascontiguousarray(renew_expires_at, dtype=np.int64)
        fid = np.ascontiguousarray(free_ids, dtype=np.uint64)
        rs = np.ascontiguousarray(report_servants, dtype=np.uint32)
        ro = np.ascontiguousarray(report_off, dtype=np.uint32)
        ri = np.ascontiguousarray(report_ids, dtype=np.uint64)
        assert len(rid) == len(rex) and (len(rs) == 0 or len(ro) == len(rs) + 1)
        assert len(rs) == 0 or int(ro[-1]) == len(ri)
        keep = [np.ascontiguousarray(requests[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        ni = np.ascontiguousarray(n_immediate, dtype=np.uint32)
        npf = np.ascontiguousarray(n_prefetch, dtype=np.uint32)
        lfor = np.ascontiguousarray(lease_for, dtype=np.int64)
        dl = np.ascontiguousarray(deadlines, dtype=np.int64)
        tg = np.ascontiguousarray(tags, dtype=np.uint64)
        assert len(ni) == n and len(npf) == n and len(lfor) == n and len(dl) == n and len(tg) == n
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        row_off = np.concatenate([[0], np.cumsum(ni.astype(np.int64) + npf)]).astype(np.int64)
        rows = max(int(row_off[-1]), 1)
        status, n_granted = np.empty(n, np.uint32), np.empty(n, np.uint32)
        out, ids = np.empty(rows, np.uint32), np.empty(rows, np.uint64)
        renewed = np.zeros(len(rid), np.uint8)
        unknown = np.zeros(len(ri), np.uint8)
        cap, rcap = max(self._max_waiting, 1), max(self._max_rows, 1)
        res_tags, res_status = np.empty(cap, np.uint64), np.empty(cap, np.uint32)
        res_n, res_first = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        res_srv, res_ids = np.empty(rcap, np.uint32), np.empty(rcap, np.uint64)
        n_leases, n_res, n_wait, n_wrows = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if env_masks is None:
            em, words = None, 1
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(ui), -1)
            words = em.shape[1]
        self._check(lib().ydc_stream_tick_rpc(
            self._h, ui.ctypes.data, ur.ctypes.data, None if em is None else em.ctypes.data, words, len(ui),
            rel.ctypes.data, len(rel), rid.ctypes.data, rex.ctypes.data, len(rid), fid.ctypes.data, len(fid),
            rs.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(rs), C.byref(soa), ni.ctypes.data, npf.ctypes.data,
            lfor.ctypes.data, dl.ctypes.data, tg.ctypes.data, n, int(now), status.ctypes.data, n_granted.ctypes.data,
            out.ctypes.data, ids.ctypes.data, renewed.ctypes.data, unknown.ctypes.data, C.byref(n_leases),
            res_tags.ctypes.data, res_status.ctypes.data, res_n.ctypes.data, res_first.ctypes.data,
            res_srv.ctypes.data, res_ids.ctypes.data, C.byref(n_res), C.byref(n_wait), C.byref(n_wrows)),
            "ydc_stream_tick_rpc")
        self._alive_shrink()
        k = n_res.value
        g = int((res_first[:k].astype(np.int64) + res_n[:k]).max()) if k else 0
        return {"status": status, "n_granted": n_granted, "row_off": row_off, "servants": out[:int(row_off[-1])],
                "task_ids": ids[:int(row_off[-1])], "renewed": renewed, "report_unknown": unknown,
                "n_leases": int(n_leases.value), "res_tags": res_tags[:k].copy(), "res_status": res_status[:k].copy(),
                "res_n_granted": res_n[:k].copy(), "res_first": res_first[:k].copy(),
                "res_servants": res_srv[:g].copy(), "res_task_ids": res_ids[:g].copy(),
                "n_waiting": int(n_wait.value), "n_waiting_rows": int(n_wrows.value)}

    def stream_caps(self):
        """The open stream's bounds (ydc_stream_caps_get) as a dict; max_tasks is an rpc stream's
        max_requests, and what the stream's mode does not have is 0."""
        caps = StreamCaps()
        self._check(lib().ydc_stream_caps_get(self._h, C.byref(caps)), "ydc_stream_caps_get")
        return {k: int(getattr(caps, k)) for k, _ in StreamCaps._fields_}

    def stream_reserve(self, **caps):
        """Grows the open stream's bounds to max(current, given) with its waiting queue and lease
        table kept (ydc_stream_reserve); keywords as the keys of stream_caps(), max_requests for
        max_tasks accepted. Returns the bounds afterwards."""
        if "max_requests" in caps:
            caps["max_tasks"] = max(int(caps.pop("max_requests")), int(caps.get("max_tasks", 0)))
        want = StreamCaps()
        for k, v in caps.items():
            if k not in dict(StreamCaps._fields_):
                raise TypeError("stream_reserve: unknown capacity %r" % k)
            setattr(want, k, int(v))
        self._check(lib().ydc_stream_reserve(self._h, C.byref(want)), "ydc_stream_reserve")
        now = self.stream_caps()
        # (the result arrays of the tick calls are sized by these)
        self._stream_caps = (now["max_updates"], now["max_releases"], now["max_tasks"])
        self._max_waiting, self._max_leases, self._max_rows = now["max_waiting"], now["max_leases"], now["max_rows"]
        return now

    def stream_snapshot(self):
        """Everything the open stream keeps on the device, and the registry, as one block of bytes
        (ydc_stream_snapshot; the format: yadcc_amd/snapshot.py)."""
        need = C.c_size_t(0)
        rc = lib().ydc_stream_snapshot(self._h, None, C.c_size_t(0), C.byref(need))
        if rc != -4:  # (YDC_ERR_CAPACITY with the size needed is the expected answer)
            self._check(rc or -1, "ydc_stream_snapshot")
        buf = C.create_string_buffer(need.value)
        self._check(lib().ydc_stream_snapshot(self._h, buf, C.c_size_t(need.value), C.byref(need)), "ydc_stream_snapshot")
        return buf.raw[:need.value]

    def _sized_blob(self, fn, what):
        """A call of ydc_stream_snapshot's shape: asked for the size, then for the bytes."""
        need = C.c_size_t(0)
        rc = fn(self._h, None, C.c_size_t(0), C.byref(need))
        if rc != -4:  # (YDC_ERR_CAPACITY with the size needed is the expected answer)
            self._check(rc or -1, what)
        buf = C.create_string_buffer(need.value)
        self._check(fn(self._h, buf, C.c_size_t(need.value), C.byref(need)), what)
        return buf.raw[:need.value]

    def stream_delta_base(self):
        """ydc_stream_snapshot's bytes, and the base a later stream_delta is taken against is kept on the
        device (ydc_stream_delta_base)."""
        return self._sized_blob(lib().ydc_stream_delta_base, "ydc_stream_delta_base")

    def stream_delta(self):
        """The delta blob from the base state to the current one, which becomes the new base
        (ydc_stream_delta; the format: yadcc_amd/snapshot.py parse_delta). YdcError "no delta base" when
        there is no base or the chain has ended: take a new stream_delta_base."""
        return self._sized_blob(lib().ydc_stream_delta, "ydc_stream_delta")

    def stream_delta_apply(self, delta):
        """Applies a delta to this standby: restored from the base's bytes, every delta since applied, never
        ticked (ydc_stream_delta_apply). A refused delta leaves the context as it was."""
        delta = bytes(delta)
        self._check(lib().ydc_stream_delta_apply(self._h, delta, C.c_size_t(len(delta))), "ydc_stream_delta_apply")

    def stream_delta_stop(self):
        """Frees the base image (ydc_stream_delta_stop)."""
        self._check(lib().ydc_stream_delta_stop(self._h), "ydc_stream_delta_stop")

    def stream_delta_inspect(self, delta=None):
        """The inspection sidecar of the delta just taken (its inserted leases' records), or with
        delta=None the full one that goes beside stream_snapshot's or stream_delta_base's bytes; both with
        the two servant columns whole (ydc_stream_delta_inspect; the format: yadcc_amd/snapshot.py
        parse_inspect_delta). Called before the next tick."""
        delta = None if delta is None else bytes(delta)
        size = C.c_size_t(0 if delta is None else len(delta))

        def fn(h, out, cap, need):
            return lib().ydc_stream_delta_inspect(h, delta, size, out, cap, need)
        return self._sized_blob(fn, "ydc_stream_delta_inspect")

    def stream_inspect_restore(self, side):
        """Switches inspection on with a full sidecar's servant columns, records and epoch, on a context in
        the very state the sidecar describes: just restored from the matching snapshot
        (ydc_stream_inspect_restore). A refused sidecar leaves the context as it was."""
        side = bytes(side)
        self._check(lib().ydc_stream_inspect_restore(self._h, side, C.c_size_t(len(side))), "ydc_stream_inspect_restore")

    def stream_delta_apply_inspected(self, delta, side):
        """stream_delta_apply on a standby with inspection on: the delta and its sidecar together
        (ydc_stream_delta_apply_inspected). A refused pair leaves the context as it was."""
        delta, side = bytes(delta), bytes(side)
        self._check(lib().ydc_stream_delta_apply_inspected(self._h, delta, C.c_size_t(len(delta)), side, C.c_size_t(len(side))),
                    "ydc_stream_delta_apply_inspected")

    def stream_restore(self, blob, **want):
        """Makes this context what the snapshotted one was (ydc_stream_restore): registry, running_tasks,
        host aliases and the open stream, its bounds max(blob's, want) — keywords as stream_reserve's.
        Returns the bounds."""
        from . import snapshot
        if "max_requests" in want:
            want["max_tasks"] = max(int(want.pop("max_requests")), int(want.get("max_tasks", 0)))
        caps = StreamCaps()
        for k, v in want.items():
            if k not in dict(StreamCaps._fields_):
                raise TypeError("stream_restore: unknown capacity %r" % k)
            setattr(caps, k, int(v))
        blob = bytes(blob)
        self._check(lib().ydc_stream_restore(self._h, blob, C.c_size_t(len(blob)), C.byref(caps) if want else None),
                    "ydc_stream_restore")
        head = snapshot.HEADER.unpack_from(blob)
        self.n_servants = int(head[7])
        self._alive = bool(head[5] & 16)
        self._alive_removals = 0
        now = self.stream_caps()
        self._stream_caps = (now["max_updates"], now["max_releases"], now["max_tasks"])
        self._max_waiting, self._max_leases, self._max_rows = now["max_waiting"], now["max_leases"], now["max_rows"]
        return now

    def stream_book_begin(self, max_book):
        """Switches the running-task book of the open leased, waiting-and-leased or rpc stream on,
        or grows it with its entries kept (ydc_stream_book_begin)."""
        self._check(lib().ydc_stream_book_begin(self._h, int(max_book)), "ydc_stream_book_begin")

    def stream_book_stage(self, servant_task_ids=None, digest_keys=None, n_ids=None):
        """The payload columns of the next accepted tick's reports, parallel to its report_ids
        (ydc_stream_book_stage); a column left out is zeros."""
        st = None if servant_task_ids is None else np.ascontiguousarray(servant_task_ids, dtype=np.uint64)
        dk = None if digest_keys is None else np.ascontiguousarray(digest_keys, dtype=np.uint64)
        if n_ids is None:
            n_ids = len(st) if st is not None else len(dk) if dk is not None else 0
        assert all(a is None or len(a) == n_ids for a in (st, dk))
        self._check(lib().ydc_stream_book_stage(self._h, _ptr(st), _ptr(dk), int(n_ids)), "ydc_stream_book_stage")

    def stream_book(self):
        """The running-task book in its order (ydc_stream_book_get): (servant_idx uint32,
        task_grant_id, servant_task_id, digest_key uint64)."""
        n = C.c_uint32(0)
        rc = lib().ydc_stream_book_get(self._h, None, None, None, None, 0, C.byref(n))
        if rc == 0:
            return np.empty(0, np.uint32), np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint64)
        cap = int(n.value)
        if cap == 0:
            self._check(rc, "ydc_stream_book_get")
        srv = np.empty(cap, np.uint32)
        gid, stid, dkey = np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint64)
        self._check(lib().ydc_stream_book_get(self._h, srv.ctypes.data, gid.ctypes.data, stid.ctypes.data,
                                              dkey.ctypes.data, cap, C.byref(n)), "ydc_stream_book_get")
        return srv, gid, stid, dkey

    def stream_book_find(self, keys):
        """Who already compiles each digest (ydc_stream_book_find): (structured array of HIT_DTYPE, one
        row per key — the LAST entry of the book with that digest_key, pos == BOOK_NOT_FOUND where
        there is none —, rebuilt: whether this call built the digest index)."""
        q = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(q), HIT_DTYPE)
        rebuilt = C.c_uint32(0)
        for at in range(0, max(len(q), 1), 1 << 24):  # (the call takes 2^24 queries)
            part, res, once = q[at:at + (1 << 24)], out[at:at + (1 << 24)], C.c_uint32(0)
            self._check(lib().ydc_stream_book_find(self._h, _ptr(part), len(part), _ptr(res), C.byref(once)),
                        "ydc_stream_book_find")
            rebuilt.value |= once.value
        return out, bool(rebuilt.value)

    def stream_book_distinct(self):
        """The book folded to one row per digest_key, the last entry winning, in the order of the
        winners' positions (ydc_stream_book_distinct): ((servant_idx uint32, task_grant_id,
        servant_task_id, digest_key uint64, count uint32), rebuilt)."""
        n, rebuilt = C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_book_distinct(self._h, None, None, None, None, None, 0, C.byref(n), C.byref(rebuilt))
        cap = int(n.value)
        if rc != 0 and cap == 0:
            self._check(rc, "ydc_stream_book_distinct")
        srv, cnt = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
        gid, stid, dkey = np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint64)
        if cap:
            again = C.c_uint32(0)
            self._check(lib().ydc_stream_book_distinct(self._h, srv.ctypes.data, gid.ctypes.data, stid.ctypes.data,
                                                       dkey.ctypes.data, cnt.ctypes.data, cap, C.byref(n),
                                                       C.byref(again)), "ydc_stream_book_distinct")
            rebuilt.value |= again.value
        return (srv, gid, stid, dkey, cnt), bool(rebuilt.value)

    def stream_alive_begin(self, expires_at=None, n=None):
        """Switches the servants' expiry column of the open leased, waiting-and-leased or rpc stream
        on (ydc_stream_alive_begin): one expires_at (int64, the ticks' clock) per servant of the
        registry; None: `n` servants that never expire until a heartbeat says otherwise."""
        e = None if expires_at is None else np.ascontiguousarray(expires_at, dtype=np.int64)
        if n is None:
            n = len(e) if e is not None else 0
        assert e is None or len(e) == n
        self._check(lib().ydc_stream_alive_begin(self._h, _ptr(e), int(n)), "ydc_stream_alive_begin")
        if not self._alive:
            self._alive_removals = 0
        self._alive = True

    def _alive_shrink(self):
        """With aliveness on, a tick may have erased servants: the row count follows (from the
        stream's running count of erased rows, a call that cannot fail)."""
        if self._alive:
            total = self.debug_alive()[2]
            self.n_servants -= total - self._alive_removals
            self._alive_removals = total

    def stream_alive_stage(self, upd_expires_at):
        """The expiries of the next accepted tick's heartbeats, parallel to its upd_idx
        (ydc_stream_alive_stage)."""
        e = np.ascontiguousarray(upd_expires_at, dtype=np.int64)
        self._check(lib().ydc_stream_alive_stage(self._h, _ptr(e) if len(e) else None, len(e)), "ydc_stream_alive_stage")

    def stream_alive_removed(self):
        """(rows the most recent accepted tick erased — ascending, in the numbering before its
        removal —, leases that went with them as orphans) (ydc_stream_alive_removed)."""
        n, orphans = C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_alive_removed(self._h, None, 0, C.byref(n), C.byref(orphans))
        if n.value == 0:
            self._check(rc, "ydc_stream_alive_removed")
            return np.empty(0, np.uint32), int(orphans.value)
        idx = np.empty(n.value, np.uint32)
        self._check(lib().ydc_stream_alive_removed(self._h, idx.ctypes.data, len(idx), C.byref(n), C.byref(orphans)),
                    "ydc_stream_alive_removed")
        return idx, int(orphans.value)

    def stream_alive(self):
        """The servants' expiry column (ydc_stream_alive_get): int64 per servant."""
        n = C.c_uint32(0)
        rc = lib().ydc_stream_alive_get(self._h, None, 0, C.byref(n))
        if n.value == 0:
            self._check(rc, "ydc_stream_alive_get")
            return np.empty(0, np.int64)
        out = np.empty(n.value, np.int64)
        self._check(lib().ydc_stream_alive_get(self._h, out.ctypes.data, len(out), C.byref(n)), "ydc_stream_alive_get")
        return out

    def debug_alive(self):
        """Tests and tools: (the host's lower bound of the smallest expires_at, ticks that asked the
        device who is due so far, servants the ticks removed so far)."""
        b, a, r = C.c_int64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(lib().ydc_debug_alive(self._h, C.byref(b), C.byref(a), C.byref(r)), "ydc_debug_alive")
        return int(b.value), int(a.value), int(r.value)

    def stream_inspect_begin(self, discovered_at=None, ever_assigned=None):
        """Switches inspection of the open leased, waiting-and-leased or rpc stream on
        (ydc_stream_inspect_begin): per servant discovered_at (int64, the ticks' clock; None: the
        previous tick's now) and ever_assigned (uint64; None: 0)."""
        d = None if discovered_at is None else np.ascontiguousarray(discovered_at, dtype=np.int64)
        e = None if ever_assigned is None else np.ascontiguousarray(ever_assigned, dtype=np.uint64)
        n = len(d) if d is not None else len(e) if e is not None else self.n_servants
        assert all(a is None or len(a) == n for a in (d, e))
        self._check(lib().ydc_stream_inspect_begin(self._h, _ptr(d), _ptr(e), int(n)), "ydc_stream_inspect_begin")

    def stream_inspect_load(self, task_id, started_at=None, env_id=None, requestor_ip=None, prefetch=None, **_):
        """Files the details of leases that exist, by id (ydc_stream_inspect_load); takes the dict
        stream_inspect_tasks returns as keywords. A column left out: the sentinel / 0."""
        ids = np.ascontiguousarray(task_id, dtype=np.uint64)
        cols = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in
                ((started_at, np.int64), (env_id, np.uint32), (requestor_ip, np.uint32), (prefetch, np.uint8))]
        assert all(a is None or len(a) == len(ids) for a in cols)
        self._check(lib().ydc_stream_inspect_load(self._h, _ptr(ids), *[_ptr(a) for a in cols], len(ids)),
                    "ydc_stream_inspect_load")

    def stream_inspect_servants(self):
        """Per servant discovered_at, ever_assigned, running_tasks, capacity_available, and the
        cluster's "totals" (dict of the five numbers DumpInternals prints) (ydc_stream_inspect_servants)."""
        n = C.c_uint32(0)
        rc = lib().ydc_stream_inspect_servants(self._h, None, None, None, None, 0, C.byref(n), None)
        if rc != -4:  # (YDC_ERR_CAPACITY with the count is the expected answer; no servants: 0)
            self._check(rc, "ydc_stream_inspect_servants")
        k = int(n.value)
        disc, ever = np.empty(k, np.int64), np.empty(k, np.uint64)
        run, avail = np.empty(k, np.uint32), np.empty(k, np.uint32)
        tot = StreamTotals()
        self._check(lib().ydc_stream_inspect_servants(self._h, _ptr(disc), _ptr(ever), _ptr(run), _ptr(avail), k,
                                                      C.byref(n), C.byref(tot)), "ydc_stream_inspect_servants")
        return {"discovered_at": disc, "ever_assigned": ever, "running_tasks": run, "capacity_available": avail,
                "totals": {f: int(getattr(tot, f)) for f, _ in StreamTotals._fields_}}

    def stream_inspect_tasks(self):
        """The lease table in id order with every lease's details (ydc_stream_inspect_tasks): dict of
        task_id, servant_idx, expires_at, zombie, started_at, env_id, requestor_ip, prefetch."""
        n = C.c_uint32(0)
        rc = lib().ydc_stream_inspect_tasks(self._h, *([None] * 8), 0, C.byref(n))
        if rc != -4:
            self._check(rc, "ydc_stream_inspect_tasks")
        k = int(n.value)
        cols = {"task_id": np.empty(k, np.uint64), "servant_idx": np.empty(k, np.uint32),
                "expires_at": np.empty(k, np.int64), "zombie": np.empty(k, np.uint8),
                "started_at": np.empty(k, np.int64), "env_id": np.empty(k, np.uint32),
                "requestor_ip": np.empty(k, np.uint32), "prefetch": np.empty(k, np.uint8)}
        self._check(lib().ydc_stream_inspect_tasks(self._h, *[_ptr(a) for a in cols.values()], k, C.byref(n)),
                    "ydc_stream_inspect_tasks")
        return cols

    def stream_outlook(self, env_id, min_version):
        """The outlook of every personality (env_id[i], min_version[i]) (ydc_stream_outlook_get): dict
        of arrays eligible, free_servants, grants_available, running_tasks, max_tasks,
        capacity_available, waiting, waiting_rows, leases, zombies (the last two OUTLOOK_UNKNOWN while
        inspection is off)."""
        env = np.ascontiguousarray(env_id, dtype=np.uint32)
        minv = np.ascontiguousarray(min_version, dtype=np.uint32)
        assert env.ndim == 1 and env.shape == minv.shape
        out = np.zeros(len(env), OUTLOOK_DTYPE)
        self._check(lib().ydc_stream_outlook_get(self._h, _ptr(env), _ptr(minv), len(env), _ptr(out)),
                    "ydc_stream_outlook_get")
        return {k: out[k].copy() for k in OUTLOOK_DTYPE.names}

    def stream_waiting(self, cap=None):
        """The waiting queue in queue order, left as it is (ydc_stream_inspect_waiting): dict of tag,
        env_id, min_version, requestor_ip, deadline, lease_for, n_immediate, n_prefetch. cap: the
        room offered (None: asked for first)."""
        n = C.c_uint32(0)
        if cap is None:
            rc = lib().ydc_stream_inspect_waiting(self._h, *([None] * 8), 0, C.byref(n))
            if rc != -4:  # (YDC_ERR_CAPACITY with the count is the expected answer; an empty queue: 0)
                self._check(rc, "ydc_stream_inspect_waiting")
            cap = int(n.value)
        cols = {"tag": np.empty(cap, np.uint64), "env_id": np.empty(cap, np.uint32),
                "min_version": np.empty(cap, np.uint32), "requestor_ip": np.empty(cap, np.uint32),
                "deadline": np.empty(cap, np.int64), "lease_for": np.empty(cap, np.int64),
                "n_immediate": np.empty(cap, np.uint32), "n_prefetch": np.empty(cap, np.uint32)}
        self._check(lib().ydc_stream_inspect_waiting(self._h, *[_ptr(a) for a in cols.values()], cap, C.byref(n)),
                    "ydc_stream_inspect_waiting")
        return {k: a[:n.value].copy() for k, a in cols.items()}

    def stream_inspect_select(self, cap, servant=None, zombie=None, expires_before=None, after_id=None, env_id=None,
                              requestor_ip=None, prefetch=None, started_before=None, unattributed=False):
        """The `cap` smallest ids among the leases that satisfy every given predicate, filtered on the
        device (ydc_stream_inspect_select): (dict of the columns stream_inspect_tasks returns, in
        ascending id order; matches: how many leases satisfy the filter). To page, pass the last id
        received as after_id. A predicate left None does not take part."""
        cap = int(cap)
        if not 0 <= cap < 2**32:
            raise ValueError("stream_inspect_select: cap %d" % cap)
        f = lease_filter(servant, zombie, expires_before, after_id, env_id, requestor_ip, prefetch, started_before,
                         unattributed)
        room = min(cap, self.stream_select_room())
        cols = {"task_id": np.empty(room, np.uint64), "servant_idx": np.empty(room, np.uint32),
                "expires_at": np.empty(room, np.int64), "zombie": np.empty(room, np.uint8),
                "started_at": np.empty(room, np.int64), "env_id": np.empty(room, np.uint32),
                "requestor_ip": np.empty(room, np.uint32), "prefetch": np.empty(room, np.uint8)}
        n, m = C.c_uint32(0), C.c_uint32(0)
        self._check(lib().ydc_stream_inspect_select(self._h, C.byref(f), *[_ptr(a) for a in cols.values()], room,
                                                    C.byref(n), C.byref(m)), "ydc_stream_inspect_select")
        return {k: a[:n.value].copy() for k, a in cols.items()}, int(m.value)

    def stream_select_room(self):
        """The rows a select can return at most, whatever cap says: the open stream's max_leases >= |L|
        (0: no stream; the library then refuses the call)."""
        caps = StreamCaps()
        if lib().ydc_stream_caps_get(self._h, C.byref(caps)) != 0:
            return 0
        return int(caps.max_leases)

    def stream_inspect_count(self, filters):
        """How many leases satisfy each of up to SELECT_MAX_FILTERS filters, from one pass over the lease
        table (ydc_stream_inspect_count). filters: LeaseFilter objects or dicts of lease_filter's
        keywords. Returns a uint32 array."""
        fs = [f if isinstance(f, LeaseFilter) else lease_filter(**f) for f in filters]
        arr = (LeaseFilter * max(len(fs), 1))(*fs)
        out = np.zeros(len(fs), np.uint32)
        self._check(lib().ydc_stream_inspect_count(self._h, arr if fs else None, len(fs), _ptr(out) if fs else None),
                    "ydc_stream_inspect_count")
        return out

    def stream_requestor_find(self, ips):
        """What each requestor holds (ydc_stream_requestor_find): (structured array of REQUESTOR_DTYPE,
        one row per queried requestor_ip — zeros where it holds nothing, the lease columns
        REQUESTOR_UNKNOWN while inspection is off or without leases —, unattributed: the leases
        granted while inspection was off, or REQUESTOR_UNKNOWN)."""
        q = np.ascontiguousarray(ips, dtype=np.uint32)
        out = np.zeros(len(q), REQUESTOR_DTYPE)
        un = C.c_uint32(0)
        for at in range(0, max(len(q), 1), 1 << 24):  # (the call takes 2^24 queries)
            part, res = q[at:at + (1 << 24)], out[at:at + (1 << 24)]
            self._check(lib().ydc_stream_requestor_find(self._h, _ptr(part) if len(part) else None, len(part),
                                                        _ptr(res) if len(part) else None, C.byref(un)),
                        "ydc_stream_requestor_find")
        return out, int(un.value)

    def stream_requestors(self):
        """Every requestor that holds a lease or waits (ydc_stream_requestor_get): (structured array
        of REQUESTOR_DTYPE sorted by requestor_ip, unattributed)."""
        n, un = C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_requestor_get(self._h, None, 0, C.byref(n), C.byref(un))
        if rc != -4:  # (YDC_ERR_CAPACITY with the count is the expected answer; nobody: 0)
            self._check(rc, "ydc_stream_requestor_get")
        out = np.zeros(int(n.value), REQUESTOR_DTYPE)
        if len(out):
            self._check(lib().ydc_stream_requestor_get(self._h, _ptr(out), len(out), C.byref(n), C.byref(un)),
                        "ydc_stream_requestor_get")
        return out[np.argsort(out["requestor_ip"], kind="stable")], int(un.value)

    def stream_withdraw_begin(self, max_withdraw):
        """Switches withdrawal by tag on for the open waiting, waiting-and-leased or rpc stream, or
        grows it (ydc_stream_withdraw_begin): room for max_withdraw tags per tick."""
        self._check(lib().ydc_stream_withdraw_begin(self._h, int(max_withdraw)), "ydc_stream_withdraw_begin")

    def stream_withdraw_stage(self, tags):
        """The tags whose waiting requests the next accepted tick takes out of the queue, answered as
        IDX_WITHDRAWN in its resolved list (ydc_stream_withdraw_stage); an empty list clears."""
        t = np.ascontiguousarray(tags, dtype=np.uint64)
        self._check(lib().ydc_stream_withdraw_stage(self._h, _ptr(t) if len(t) else None, len(t)),
                    "ydc_stream_withdraw_stage")

    def stream_withdraw_result(self):
        """(entries removed per tag staged for the most recent accepted tick, in the staged order;
        entries removed in all) (ydc_stream_withdraw_result)."""
        n, total = C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_withdraw_result(self._h, None, 0, C.byref(n), C.byref(total))
        if n.value == 0:
            self._check(rc, "ydc_stream_withdraw_result")
            return np.empty(0, np.uint32), int(total.value)
        counts = np.empty(n.value, np.uint32)
        self._check(lib().ydc_stream_withdraw_result(self._h, counts.ctypes.data, len(counts), C.byref(n),
                                                     C.byref(total)), "ydc_stream_withdraw_result")
        return counts, int(total.value)

    def stream_quota_begin(self, max_overrides=0):
        """Switches the cap per requestor on for the open waiting-and-leased or rpc stream with
        inspection on, or grows it (ydc_stream_quota_begin): room for max_overrides per-requestor caps.
        Every cap is QUOTA_UNLIMITED until stream_quota_set."""
        self._check(lib().ydc_stream_quota_begin(self._h, int(max_overrides)), "ydc_stream_quota_begin")

    def stream_quota_set(self, default_cap, overrides=None):
        """The caps from the next accepted tick on (ydc_stream_quota_set): default_cap for everybody,
        overrides a dict (or pairs) requestor_ip -> cap. A request whose requestor has no room is
        answered IDX_OVER_QUOTA."""
        pairs = list(overrides.items()) if isinstance(overrides, dict) else list(overrides or ())
        ips = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
        caps = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint32)
        self._check(lib().ydc_stream_quota_set(self._h, int(default_cap), _ptr(ips) if len(ips) else None,
                                               _ptr(caps) if len(caps) else None, len(ips)), "ydc_stream_quota_set")

    def stream_quota_result(self):
        """(admitted n_immediate, admitted n_prefetch, rows clipped, requests refused) of the most recent
        accepted tick, per new request in the caller's order (ydc_stream_quota_result); outside rpc mode
        the first is 0 / 1 and the second zeros."""
        n, clipped, refused = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_quota_result(self._h, None, None, 0, C.byref(n), C.byref(clipped), C.byref(refused))
        if n.value == 0:
            self._check(rc, "ydc_stream_quota_result")
        imm, pre = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(lib().ydc_stream_quota_result(self._h, imm.ctypes.data, pre.ctypes.data, len(imm), C.byref(n),
                                                      C.byref(clipped), C.byref(refused)), "ydc_stream_quota_result")
        return imm, pre, int(clipped.value), int(refused.value)

    def stream_quota_fair(self, mode, pool=0, floor_cap=0):
        """The fair-share level of the open stream's quota from the next accepted tick on
        (ydc_stream_quota_fair): mode FAIR_REGISTRY with pool percent of the registry's capacity,
        FAIR_FIXED with pool rows, or FAIR_OFF. A requestor without an override is capped at
        min(default_cap, max(level, floor_cap)), the level found by the tick itself."""
        self._check(lib().ydc_stream_quota_fair(self._h, int(mode), int(pool), int(floor_cap)), "ydc_stream_quota_fair")

    def stream_quota_fair_result(self):
        """The level of the most recent accepted tick and what it was found from
        (ydc_stream_quota_fair_result): a dict of ydc_fair_result's fields."""
        r = FairResult()
        self._check(lib().ydc_stream_quota_fair_result(self._h, C.byref(r)), "ydc_stream_quota_fair_result")
        return {k: int(getattr(r, k)) for k, _ in FairResult._fields_}

    def stream_depart_begin(self, max_depart):
        """Switches the departure of requestors on for the open leased, waiting-and-leased or rpc stream
        with inspection on, or grows it (ydc_stream_depart_begin): room for max_depart requestors per
        tick."""
        n = _depart_count(max_depart, "max_depart")
        self._check(lib().ydc_stream_depart_begin(self._h, n), "ydc_stream_depart_begin")

    def stream_depart_stage(self, requestors):
        """The requestors whose leases the next accepted tick frees and whose waiting requests it lets
        run out (ydc_stream_depart_stage); an empty list clears. Ids as the requestor_ip column carries
        them: whole numbers in [0, 2^32)."""
        r = _depart_keys(requestors)
        self._check(lib().ydc_stream_depart_stage(self._h, _ptr(r) if len(r) else None, len(r)),
                    "ydc_stream_depart_stage")

    def stream_depart_result(self):
        """(rows of DEPART_DTYPE, one per requestor staged for the most recent accepted tick in the staged
        order; leases freed in all; entries of W taken out in all) (ydc_stream_depart_result)."""
        n, leases, waiting = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        rc = lib().ydc_stream_depart_result(self._h, None, 0, C.byref(n), C.byref(leases), C.byref(waiting))
        if n.value == 0:
            self._check(rc, "ydc_stream_depart_result")
            return np.zeros(0, DEPART_DTYPE), int(leases.value), int(waiting.value)
        out = np.zeros(n.value, DEPART_DTYPE)
        self._check(lib().ydc_stream_depart_result(self._h, out.ctypes.data_as(C.POINTER(DepartCount)), len(out),
                                                   C.byref(n), C.byref(leases), C.byref(waiting)),
                    "ydc_stream_depart_result")
        return out, int(leases.value), int(waiting.value)

    def stream_usage_begin(self, quantum, want_requestors=0):
        """Switches the usage accounting on for the open leased, waiting-and-leased or rpc stream with
        inspection on (ydc_stream_usage_begin): every tick charges the leases and waiting requests it
        finds for the quanta (of `quantum` clock units) since the previous tick. Called again with the
        same quantum it only grows the table to want_requestors."""
        q = int(quantum)
        if not -(1 << 63) <= q < 1 << 63:
            raise ValueError("quantum %d does not fit int64" % q)
        self._check(lib().ydc_stream_usage_begin(self._h, q, _depart_count(want_requestors, "want_requestors")),
                    "ydc_stream_usage_begin")

    def stream_usage_get(self, reset=False):
        """(rows of USAGE_DTYPE IN NO SPECIFIED ORDER, the totals as a dict) (ydc_stream_usage_get). reset:
        the table and the totals are emptied behind the copy."""
        n, tot = C.c_uint32(0), UsageTotals()
        # (the row count first, without a reset: a table with rows answers YDC_ERR_CAPACITY and *out_n)
        rc = lib().ydc_stream_usage_get(self._h, None, 0, C.byref(n), C.byref(tot), 0)
        out = np.zeros(n.value, USAGE_DTYPE)
        if n.value or (reset and not rc):
            rc = lib().ydc_stream_usage_get(self._h, out.ctypes.data if n.value else None, len(out), C.byref(n),
                                            C.byref(tot), USAGE_RESET if reset else 0)
        self._check(rc, "ydc_stream_usage_get")
        return out, {k: int(getattr(tot, k)) for k, _ in UsageTotals._fields_}

    def stream_usage_find(self, requestors):
        """Rows of USAGE_DTYPE, one per queried requestor in the queried order; a requestor the table does
        not hold is a row of zeros (ydc_stream_usage_find)."""
        r = _depart_keys(requestors)
        out = np.zeros(len(r), USAGE_DTYPE)
        self._check(lib().ydc_stream_usage_find(self._h, _ptr(r) if len(r) else None, len(r),
                                                out.ctypes.data if len(r) else None), "ydc_stream_usage_find")
        return out

    def stream_usage_load(self, rows, totals=None):
        """Adds rows of USAGE_DTYPE to the table, duplicates together, and what `totals` (a dict with
        unattributed_time, quanta, ticks) names to the totals (ydc_stream_usage_load)."""
        a = np.ascontiguousarray(rows, dtype=USAGE_DTYPE)
        tot = None
        if totals is not None:
            tot = UsageTotals()
            for k in ("unattributed_time", "quanta", "ticks"):
                setattr(tot, k, int(totals.get(k, 0)) & ((1 << 64) - 1))
        self._check(lib().ydc_stream_usage_load(self._h, a.ctypes.data if len(a) else None, len(a),
                                                C.byref(tot) if tot is not None else None), "ydc_stream_usage_load")

    def stream_leases(self):
        """Snapshot of the lease table in id order (ydc_stream_leases_get): (task_ids uint64,
        servant_idx uint32, expires_at int64, zombie uint8)."""
        cap = max(self._max_leases, 1)
        ids, srv = np.empty(cap, np.uint64), np.empty(cap, np.uint32)
        exp, zom = np.empty(cap, np.int64), np.empty(cap, np.uint8)
        n = C.c_uint32(0)
        self._check(lib().ydc_stream_leases_get(self._h, ids.ctypes.data, srv.ctypes.data, exp.ctypes.data,
                                                zom.ctypes.data, cap, C.byref(n)), "ydc_stream_leases_get")
        k = n.value
        return ids[:k].copy(), srv[:k].copy(), exp[:k].copy(), zom[:k].copy()

    def stream_waiting_take(self):
        """Empties the waiting queue; returns its tags in queue order (ydc_stream_waiting_take)."""
        n = C.c_uint32(0)
        out = np.empty(max(self._max_waiting, 1), np.uint64)
        self._check(lib().ydc_stream_waiting_take(self._h, out.ctypes.data, len(out), C.byref(n)),
                    "ydc_stream_waiting_take")
        return out[:n.value].copy()

    def stream_tick(self, upd_idx, upd_rows, release_idx, tasks, env_masks=None):
        """upd_rows: numpy structured array of ROW_DTYPE (one heartbeat per entry of upd_idx);
        release_idx: servant index of every freed grant; tasks: dict of request columns.
        env_masks: optional (len(upd_idx), env_words) uint64 array — the heartbeats' environment
        sets on a registry with more than 64 digests (ydc_stream_tick_wide).
        Returns the servant index (or IDX_*) of every request."""
        ui = np.ascontiguousarray(upd_idx, dtype=np.uint32)
        if len(ui):
            self.n_servants = max(self.n_servants, int(ui.max()) + 1)
        ur = np.ascontiguousarray(upd_rows, dtype=ROW_DTYPE)
        rel = np.ascontiguousarray(release_idx, dtype=np.uint32)
        keep = [np.ascontiguousarray(tasks[k], dtype=np.uint32)
                for k in ("env_id", "min_version", "requestor_ip")]
        n = len(keep[0])
        soa = TaskSoA(*[a.ctypes.data for a in keep])
        out = np.empty(n, np.uint32)
        if env_masks is None:
            self._check(lib().ydc_stream_tick(self._h, ui.ctypes.data, ur.ctypes.data, len(ui),
                                              rel.ctypes.data, len(rel), C.byref(soa), n,
                                              out.ctypes.data), "ydc_stream_tick")
        else:
            em = np.ascontiguousarray(env_masks, dtype=np.uint64).reshape(len(ui), -1)
            self._check(lib().ydc_stream_tick_wide(self._h, ui.ctypes.data, ur.ctypes.data,
                                                   em.ctypes.data, em.shape[1], len(ui),
                                                   rel.ctypes.data, len(rel), C.byref(soa), n,
                                                   out.ctypes.data), "ydc_stream_tick_wide")
        return out

    def stream_buffers(self, max_updates=None, max_releases=None, max_tasks=None):
        """numpy views of the page-locked arrays a tick is staged in (ydc_stream_buffers_get): fill
        them in place and call stream_tick_inplace — nothing is copied on either side. The views
        have the capacities stream_begin was given (arguments, if any, may only ask for less)."""
        caps = self._stream_caps
        want = (max_updates, max_releases, max_tasks)
        if any(w is not None and w > c for w, c in zip(want, caps)):
            raise YdcError("stream_buffers%r: beyond the capacities of stream_begin%r" % (want, caps))
        max_updates, max_releases, max_tasks = [c if w is None else w for w, c in zip(want, caps)]
        class _B(C.Structure):
            _fields_ = [(k, C.c_void_p) for k in ("upd_idx", "upd_rows", "release_servant_idx", "env_id",
                                                   "min_version", "requestor_ip", "out_servant_idx")]
        b = _B()
        self._check(lib().ydc_stream_buffers_get(self._h, C.byref(b)), "ydc_stream_buffers_get")

        def view(p, n, dt):
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(p)
            return np.frombuffer(buf, dtype=dt, count=n)
        self._stream_views = {
            "upd_idx": view(b.upd_idx, max_updates, np.uint32), "upd_rows": view(b.upd_rows, max_updates, ROW_DTYPE),
            "release_idx": view(b.release_servant_idx, max_releases, np.uint32),
            "env_id": view(b.env_id, max_tasks, np.uint32), "min_version": view(b.min_version, max_tasks, np.uint32),
            "requestor_ip": view(b.requestor_ip, max_tasks, np.uint32), "out": view(b.out_servant_idx, max_tasks, np.uint32)}
        return self._stream_views

    def stream_tick_inplace(self, n_upd, n_rel, n_tasks):
        """One tick whose data already lies in stream_buffers(); the answers are in views["out"][:n_tasks]."""
        v = self._stream_views
        soa = TaskSoA(v["env_id"].ctypes.data, v["min_version"].ctypes.data, v["requestor_ip"].ctypes.data)
        self._check(lib().ydc_stream_tick(self._h, v["upd_idx"].ctypes.data, v["upd_rows"].ctypes.data, n_upd,
                                          v["release_idx"].ctypes.data, n_rel, C.byref(soa), n_tasks,
                                          v["out"].ctypes.data), "ydc_stream_tick")
        return v["out"][:n_tasks]

    def stream_end(self):
        self._check(lib().ydc_stream_end(self._h), "ydc_stream_end")
        self._max_waiting = 0
        self._alive = False

    def set_profiling(self, on):
        self._check(lib().ydc_set_profiling(self._h, int(on)), "ydc_set_profiling")

    def kernel_profile(self):
        """{"kernel": [launches, total_ms]} of the last dispatch (profiling must be on)."""
        import json
        return json.loads(lib().ydc_kernel_profile(self._h).decode() or "{}")

    def stats(self):
        st = Stats()
        self._check(lib().ydc_get_stats(self._h, C.byref(st)), "ydc_get_stats")
        return st.as_dict()
