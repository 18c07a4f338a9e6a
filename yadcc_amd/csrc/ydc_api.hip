// ydc_api.hip — the extern "C" boundary (include/yadcc_dispatch.h): context,
// resident servant registry, per-batch launch sequence. gfx950 only; there is
// no CPU fallback — without a device every call fails with YDC_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is resolved with dlopen at ydc_group_init

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <numeric>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/yadcc_dispatch.h"
#include "dispatch_core.h"
#include "host_tables.h"
#include "lane_rule.h"
#include "occupancy_plan.h"
#include "registry_mirror.h"
#include "shard_plan.h"
#include "kernels.h"
#include "wait_queue.h"
#include "lease_table.h"
#include "rpc_stream.h"
#include "wait_lease.h"
#include "running_book.h"
#include "book_index.h"
#include "servant_alive.h"
#include "stream_inspect.h"
#include "stream_select.h"
#include "stream_outlook.h"
#include "requestor_index.h"
#include "admit_clip.h"
#include "stream_delta.h"
#include "stream_delta_codec.h"
#include "stream_inspect_delta.h"
#include "stream_inspect_delta_codec.h"
#include "stream_snapshot.h"
#include "stream_snapshot_codec.h"
#include "stream_depart.h"
#include "stream_fair.h"
#include "stream_quota.h"
#include "stream_usage.h"
#include "stream_withdraw.h"
#include "tick_kernel.h"
#include "usage_quanta.h"

using namespace ydc;

namespace {

// Owns one device allocation (freed with whatever holds it: the context, a stream, the group).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(n, 16);
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Owns one page-locked allocation in the same way. z: the block's device address where it is
// mapped (the default flags), NULL where it is not.
struct PinnedBuf {
  uint8_t *p = nullptr, *z = nullptr;
  size_t cap = 0;  // bytes
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept { *this = std::move(o); }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr), z = std::exchange(o.z, nullptr), cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  // Grow only; the contents are not kept.
  hipError_t reserve(size_t bytes, unsigned flags = hipHostMallocCoherent | hipHostMallocMapped) {
    if (bytes <= cap) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(bytes, 16);
    hipError_t e = hipHostMalloc((void**)&p, want, flags);
    if (e != hipSuccess) p = nullptr;
    else if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void**)&z, p, 0);
    if (e == hipSuccess) cap = want;
    else release();
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = z = nullptr;
    cap = 0;
  }
};

// A PinnedBuf that holds objects of one type: the block at its host address, dev() at the device's.
template <typename T>
struct PinnedAs : PinnedBuf {
  T* get() const { return (T*)p; }
  T* dev() const { return (T*)z; }
  operator T*() const { return get(); }
  T* operator->() const { return get(); }
};

// Own one event / one stream in the same way; created at their first use.
struct OwnedEvent {
  hipEvent_t e = nullptr;
  OwnedEvent() = default;
  OwnedEvent(const OwnedEvent&) = delete;
  OwnedEvent& operator=(const OwnedEvent&) = delete;
  OwnedEvent(OwnedEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  ~OwnedEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() = default;
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  ~OwnedStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

}  // namespace

namespace {
// Sizes, workspace views and kernel argument blocks of one batch (plan_batch).
struct BatchPlan {
  uint32_t N = 0, S = 0, C = 0, W = 1, slot_bound = 0, n_tiles = 1, cs = 64, K = 0;
  uint32_t key_passes = 0, cls_passes = 0, cls_bits = 0, rshift = 4, init_fill = 8, sort_items = 8;
  uint32_t ring_total = 2048;  // entries of all rings of a matching wave (x 8 B of LDS)
  bool dense = false;  // the matching kernel's 4-waves-per-SIMD build (match_kernel.h: OCC)
  uint32_t fused_cls_bits = 0;  // class partition folded into the last key pass (kernels.h)
  uint32_t gbits = 0;  // != 0: the sort's values carry the class above gbits slot bits (SortIn)
  uint32_t slot_bound_glob = 0, win_margin = 0;  // (sharded sort: slot_bound is the window's)
  bool key32 = true, any_shared = false, use_generic = false, wave_path = false;
  bool packed = false;  // the sort moves 8-byte (key, value) records (32-bit keys)
  bool win = false;  // multi-GPU with a sharded sort: this rank only holds a key window of the slots
  // Bin sort (bin_sort.h) instead of the radix sort: n_bins equal bins over the key space.
  bool fuse01 = false;  // the launch of matching pass 0 is pass 1 as well (no launch for pass 1)
  bool wide_lists = false;  // > 256 classes with short eligible-class rows: k_sim_wide's list form
  bool binsort = false;
  bool zone = false;            // workgroup 0 of the launch of pass 0 walks the tier's end (zone_guess.h)
  bool zone_eligible = false;   // ... or would, if zone_decide had found it worth its while
  uint32_t n_bins = 0, bin_shift = 0, bin_slot_bits = 0, bin_cls_bits = 0;
  uint32_t bin_group = 0, bin_tiles = 0;  // servants per slot tile, slot tiles (k_front_bins)
  uint32_t bin_threads = kBinThreadsWide;  // width of a k_bin_sort workgroup (occupancy_plan.h)
  ServantTable sv{};
  ClassLists L{};
  TaskTable T{};
  MatchBuffers mb{};
  const uint32_t* rank_to_g = nullptr;  // slots in key order (before the class partition)
  uint32_t rank_stride = 1;             // 2: rank_to_g are the values of 8-byte sort records
  SharedIpTable shared{};  // pos_last != NULL: some host runs several servants
};

// The sections of a streaming tick's staging arena (stream_begin lays them out): heartbeat
// indexes and rows, released slots, the three request columns and, in waiting mode, the new
// requests' deadlines and tags and the tick's clock (NULL in a plain context); in leased mode the
// requests' lease expiries (with a waiting queue as well: their lease durations), the renewals,
// the frees by id, the servant reports (CSR) and the tick's scalars (NULL in any other context).
struct TickArena {
  uint32_t* upd_idx;
  ydc_servant_row* upd_rows;
  uint32_t* rel;
  uint32_t *env, *minv, *ip;
  int64_t* dl;
  uint64_t* tag;
  int64_t* now;
  int64_t* lexp;
  unsigned long long* ren_id;
  int64_t* ren_exp;
  unsigned long long* free_id;
  uint32_t *rep_srv, *rep_off;
  unsigned long long* rep_id;
  LeaseHdr* lh;
  uint32_t *nimm, *npre;  // rpc mode: grants asked for per request (NULL in any other context)
  unsigned long long *bk_stid, *bk_dkey;  // with a running-task book: the reports' payload columns, beside rep_id
  int64_t* upd_exp;  // leased modes: the heartbeats' expiries, beside upd_idx (read only with aliveness on)
  uint64_t* wd_tag;  // with withdrawal: the tick's staged tags (sorted, unique) and their number
  uint32_t* wd_n;
  uint32_t* q_n;  // with a quota: the tick's number of new requests (the columns behind it are padding)
  uint32_t* dp_ip;  // with departure: the tick's staged requestors (sorted, unique) and their number
  uint32_t* dp_n;
};
}  // namespace

struct ydc_context {
  int device = 0;
  // The first member, so the last to go: everything below is released while it still exists.
  OwnedStream own_stream;        // the context's stream where the caller brought none
  hipStream_t stream = nullptr;  // the caller's, or own_stream
  uint32_t max_servants = 0, max_tasks = 0, max_slots = 0;
  std::string last_error;

  // Host mirror of the registry columns the derived tables need, and the host aliases.
  RegistryMirror reg;
  uint32_t n_parts = 1;         // independent parts of the registry (host_tables.h)
  HostTables tables;
  KeyFormat kf{};
  bool tables_dirty = true;

  // Resident registry (its six per-servant columns: kRegCols, below).
  DevBuf<uint32_t> d_version, d_nproc, d_load, d_max_tasks, d_running, d_flags, d_class_of;
  DevBuf<uint32_t> d_spare[6];  // ydc_remove_servants compacts into these (kRegCols' order), then swaps
  DevBuf<uint32_t> d_ip_hash, d_ip_filter;
  DevBuf<uint32_t> d_bin_tile_start, d_bin_tile_base;  // slot tiles of the bin sort's front (host_tables.h)
  DevBuf<uint32_t> d_ip_sorted, d_ip_servant, d_cls_ver, d_ver_sorted, d_cls_comp, d_part_base;
  DevBuf<uint64_t> d_cls_env, d_env_ver_mask;
  DevBuf<uint8_t> d_cls_single;

  // Per-batch workspace.
  DevBuf<uint32_t> d_slot_base, d_cls_begin, d_vals[2], d_hist, d_row_total, d_tile_first;
  DevBuf<uint64_t> d_keys[2];  // viewed as u32 when the key fits
  DevBuf<uint16_t> d_cls_by_g;
  DevBuf<uint32_t> d_owner;     // servant of every slot (generation order)
  DevBuf<uint32_t> d_rank_to_g; // global rank -> slot when the class pass is fused into the sort
  DevBuf<unsigned long long> d_zone_box;  // zone_walk's granules: header + a row of cursors per chunk
  DevBuf<uint32_t> d_binbase, d_binruns;  // bin sort: starts of the bins per class, run table of the slot tiles
  DevBuf<uint32_t> d_level_tab;           // bin sort: class-list positions at every 64th global rank
  DevBuf<uint32_t> d_elig_off, d_elig_cls, d_row_of;  // > 256 classes: eligible-class lists, the requests' rows
  DevBuf<uint64_t> d_mask;
  DevBuf<uint32_t> d_self_lo, d_self_hi, d_chunk_consuming, d_before, d_slot_of, d_pos_last;
  DevBuf<uint32_t> d_chunk_tail;  // consuming requests among the last kWarmUp of every chunk
  DevBuf<uint32_t> d_running_out;
  DevBuf<ClassState> d_guess[1], d_endst, d_checkpoint, d_early;
  DevBuf<unsigned long long> d_claim, d_hand;  // d_hand: hand-off granules of the pass 0 + 1 launch
  uint32_t round_hint = 3;  // passes to pre-launch before looking at the outcome

  // Pipelined batches (ydc_dispatch_device_async / ydc_dispatch_wait): up to two batches are
  // enqueued before the host looks at the outcome of the older one.
  struct Pending {
    bool active = false, rerun = false;
    BatchPlan plan;
    ydc_task_soa tk{};
    uint32_t n = 0, flags = 0, launched = 0;
    uint32_t* out_idx = nullptr;
    double* out_util = nullptr;
    uint32_t* out_running = nullptr;
    PinnedAs<DeviceParams> h_outcome;  // where k_finalize stores the batch's outcome
    OwnedEvent ev;
    LaneBatch lb;  // what the lane rule knows of it (lb.lane: the lane its launches are on)
    uint64_t lb_epoch = 0;  // lane0_epoch when it was enqueued
  } pend[2];
  uint32_t pend_head = 0, pend_count = 0;
  uint64_t pipeline_misses = 0;

  // Lane 1 (lane_rule.h): a second stream and a second instance of everything a batch writes on the
  // device, so that a pipelined batch which does not depend on the outstanding one runs beside it
  // instead of behind it. Made at the first batch sent there. While such a batch is enqueued
  // (LaneScope) its members stand in the context's own — every launch site reads c->stream, c->d_prm
  // and the workspace as ever — and the context's wait here; at any other time this is lane 1's.
  struct Lane {
    OwnedStream own;
    hipStream_t stream = nullptr;
    DevBuf<DeviceParams> d_prm;  // its own counters, latch and batch number (its granules' stamps)
    DevBuf<uint32_t> d_slot_base, d_cls_begin, d_vals[2], d_hist, d_row_total, d_tile_first;
    DevBuf<uint64_t> d_keys[2];
    DevBuf<uint16_t> d_cls_by_g;
    DevBuf<uint32_t> d_owner, d_rank_to_g;
    DevBuf<unsigned long long> d_zone_box;
    DevBuf<uint32_t> d_binbase, d_binruns, d_level_tab, d_row_of;
    DevBuf<uint32_t> d_bin_tile_base, d_part_base;  // (sized with the derived tables, written by every batch)
    DevBuf<uint64_t> d_mask;
    DevBuf<uint32_t> d_self_lo, d_self_hi, d_chunk_consuming, d_before, d_slot_of, d_pos_last, d_chunk_tail;
    DevBuf<uint32_t> d_running_out;
    DevBuf<ClassState> d_guess[1], d_endst, d_checkpoint, d_early;
    DevBuf<unsigned long long> d_claim, d_hand;
    DevBuf<ClassRun> d_runs;
    DevBuf<uint8_t> d_dirty;
  };
  std::unique_ptr<Lane> lane1;
  bool opt_lanes = true;       // (lanes=0: every batch on lane 0)
  // The host has seen a lane-0 batch complete since anything but a pipelined batch last used the
  // context's stream (a registry upload or update, a release, rebuild_tables, ...): what lane 1
  // reads of the registry and its tables is in place, with no event between the lanes.
  // As two counts: such uses so far, and how many of them the last lane-0 batch seen complete was
  // enqueued behind (Pending::lb_epoch). Settled when they are equal.
  uint64_t lane0_epoch = 1, lane0_seen = 0;
  bool lane0_settled() const { return lane0_seen == lane0_epoch; }
  uint64_t lane1_batches = 0;  // ydc_debug_pipeline

  // Multi-GPU group (ydc_group_*): this context is one rank of a sharded dispatcher.
  // One way of exchanging between the ranks (an all-gather a handful of times per matching pass,
  // a few hundred bytes to S*4 bytes per rank). Chosen once, when the group is made; whoever
  // exchanges asks the record, nobody looks at what it is made of. Its destructor gives back
  // everything the transport took. The implementations are with the ydc_group_* entry points.
  struct Transport {
    virtual ~Transport() = default;
    virtual int kind() const = 0;  // YDC_TRANSPORT_*
    // recv[r * bytes ..) = rank r's send[0, bytes), ordered behind c->stream.
    virtual int gather(ydc_context* c, const void* send, void* recv, size_t bytes) = 0;
    // Waits for the stream; an error where an exchange so far did not deliver every peer's data.
    // Whoever turns gathered words into sizes or inputs on the host asks here first.
    virtual int settled(ydc_context* c);
    // The transport's own count of the ranks, where it keeps one (ydc_group_size).
    virtual int count(ydc_context*, int*) { return YDC_OK; }
  };
  struct Group {
    int rank = 0, n_ranks = 0;  // n_ranks == 0: not in a group
    // (between ydc_group_ipc_export and ydc_group_init_ipc: the mailbox with this rank's own
    // blocks, and n_ranks == 0)
    std::unique_ptr<Transport> via;
    // Device buffers of the sharded batches. They live as long as the group: group_release
    // replaces the record with a fresh one, so a buffer added here is given back with the rest.
    struct Workspace {
      DevBuf<uint32_t> d_totals, d_meta, d_base, d_delta, d_deltas;
      DevBuf<ClassState> d_bound_local, d_send, d_bounds;
      // Sharded sort (k_window): key-count table, per-servant windows, local prefix, class lists
      // of the whole registry, local -> registry-wide list position shifts, the ranks' windows.
      DevBuf<uint32_t> d_cum, d_r_first, d_lbase, d_cls_begin_glob, d_shift, d_winrec, d_winall;
      DevBuf<uint32_t> d_pad, d_gather, d_all[3], d_all_idx;  // replicated fallback (whole batch)
      DevBuf<double> d_all_util;
    } ws;
    // What follows outlives a group: it stays for the next one, or goes with the context.
    PinnedAs<ClassState> h_bounds;   // page-locked (debug_sim's look at the ranks' records)
    uint32_t margin_scale = 1;       // doubled after a batch whose window missed
    uint64_t windowed_batches = 0, window_misses = 0;  // ydc_get_stats: shard_sort_batches / _misses
    uint32_t passes = 0;             // of the last sharded batch
    uint32_t pass_hint = 3;          // passes to pre-launch before looking at the outcome
    // Mailbox time-out (YDC_TUNE ipc_timeout_ms, read at every export; the slot size is read there
    // too and is kept by the mailbox alone).
    unsigned long long mailbox_timeout_ticks = 30ull * 100000000ull;
  } group;

  // Streaming mode (ydc_stream_*): one tick = row updates + slot releases + one
  // committed batch, replayed from a captured graph.
  struct Stream {
    bool active = false, stale = true;
    // The stream's bounds, once. A part the mode lacks has 0 everywhere, so they say the mode as
    // well (rpc mode: max_tasks is max_requests). max_book: the running-task book's (0: none).
    ydc_stream_caps caps{};
    uint32_t max_book = 0;
    uint32_t max_withdraw = 0;  // tags one tick can withdraw (ydc_stream_withdraw_begin; 0: the capability is off)
    uint32_t max_depart = 0;  // requestors one tick can dismiss (ydc_stream_depart_begin; 0: the capability is off)
    bool waiting() const { return caps.max_waiting != 0; }
    bool leased() const { return caps.max_leases != 0; }
    bool rpc() const { return caps.max_rows != 0; }
    uint32_t passes = 0;
    // What is sized by the bounds is laid out by stream_alloc and, when the stream grows, filled
    // by stream_migrate from the old one; what is sized by the registry (d_rep_tick, `alive`,
    // `inspect`) moves to the grown stream as it is (stream_regrow).
    // One pinned staging arena for everything a tick brings (TickArena) and its device mirror,
    // which the ticks that run eagerly copy it to. Its sections three times: at their host
    // addresses, in the mirror, and as the kernels of the captured step see the page-locked
    // arena when they read it in place (no H2D copy node).
    PinnedBuf h_in;
    DevBuf<uint8_t> d_in;
    size_t in_bytes = 0;
    TickArena h{}, d{}, z{};
    PinnedBuf h_place;                            // the placement, page-locked
    uint32_t *h_out = nullptr, *z_out = nullptr;  // ... at its host and device addresses
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    BatchPlan plan;
    // COMMIT without a copy node (commit_swap): the step exists twice, captured with the two
    // running_tasks columns in either role; a tick that took effect makes its output THE column
    // and the next tick replays the other capture. run_a / run_b: the column each one reads.
    hipGraph_t graph_b = nullptr;
    hipGraphExec_t exec_b = nullptr;
    BatchPlan plan_b;
    const uint32_t *run_a = nullptr, *run_b = nullptr;
    bool swaps = false;
    bool eager_only = false;  // the registry's batches cannot be captured (> 256 classes): every tick runs eagerly
    // Passes to capture: one more than the last eager batch needed, to begin with; after 64
    // ticks that all needed fewer, exactly the most any of them needed (a pre-launched pass
    // that finds nothing to do still costs a launch); more again after a tick that ran out.
    uint32_t want_passes = 0, window_max = 0, window_ticks = 0;
    // Waiting mode (ydc_stream_begin_waiting; wait_queue.h): the queue W of requests that found
    // no free servant, in HBM, and the tick's batch columns [max_waiting | max_tasks] the gather
    // builds in front of the batch. !waiting(): a plain context (none of this exists).
    uint32_t n_waiting = 0;  // |W| after the last tick (the outcome block's, kept here)
    int64_t last_now = INT64_MIN;
    DevBuf<uint8_t> d_wait;
    WaitCols wq{}, wt{};  // W; the tick's batch
    uint32_t* wt_out = nullptr;  // placement of the batch (k_finalize -> k_wait_compact)
    WaitState* ws = nullptr;
    unsigned long long* lookback = nullptr;
    uint32_t lookback_n = 0;
    PinnedBuf h_wres;  // page-locked: resolved tags | resolved answers | outcome
    uint64_t *h_res_tag = nullptr, *z_res_tag = nullptr;
    uint32_t *h_res_idx = nullptr, *z_res_idx = nullptr;
    WaitOutcome *h_wout = nullptr, *z_wout = nullptr;
    // Waiting and leased at once (ydc_stream_begin_waiting_leased; wait_lease.h): both of the above
    // and below exist, plus the lease durations of W and of the batch and the resolved entries' task
    // ids (page-locked, beside the resolved tags). wl.t_for == NULL: not such a context.
    WaitLeaseCols wl{};
    unsigned long long* h_res_id = nullptr;
    // Leased mode (ydc_stream_begin_leased; lease_table.h): the lease table L in HBM, the placement
    // of the tick's batch in front of k_lease_grant, and the page-locked results. !leased(): not a
    // leased context (none of this exists). lookback / lookback_n above serve k_lease_grant.
    uint32_t n_leases = 0;    // |L| after the last tick (the outcome block's, kept here)
    uint32_t lease_tick = 0;  // number of the last tick that was staged
    DevBuf<uint8_t> d_lease;
    LeaseCols lt{};
    LeaseState* ls = nullptr;
    uint32_t* ren_slot = nullptr;
    uint32_t* lt_out = nullptr;     // placement of the batch (k_finalize -> k_lease_grant)
    DevBuf<uint32_t> d_rep_tick;    // per servant: the last tick it reported in
    PinnedBuf h_lres;               // page-locked: task ids | renewed | report_unknown | outcome
    unsigned long long *h_task_id = nullptr, *z_task_id = nullptr;
    uint8_t *h_renewed = nullptr, *z_renewed = nullptr, *h_unknown = nullptr, *z_unknown = nullptr;
    LeaseOutcome *h_lout = nullptr, *z_lout = nullptr;
    // "Each servant at most once per list", checked by the host: a stamp per servant and the stamp
    // of the list being looked at (one more per look, refused ticks included).
    struct OnceMarks {
      std::vector<uint32_t> seen;
      uint32_t mark = 0;
      void begin(size_t n_servants) {
        if (seen.size() < n_servants) seen.resize(n_servants, 0);
        if (++mark == 0) {
          std::fill(seen.begin(), seen.end(), 0u);
          mark = 1;
        }
      }
      bool first(uint32_t s) { return std::exchange(seen[s], mark) != mark; }
    };
    OnceMarks rep_once;  // over a tick's report list
    // With inspection: the detail records beside L's slots (stream_inspect.h: a 16-byte record and a
    // prefetch byte per slot). Sized by the table: stream_migrate files them again with their leases.
    DevBuf<uint4> d_insp_rec;
    DevBuf<uint8_t> d_insp_pre;
    // RPC mode (ydc_stream_begin_rpc; rpc_stream.h): a waiting and leased context whose request rows
    // and entries of W are RPCs asking for several grants. max_tasks is max_requests there; the
    // batch is the max_rows expanded rows (wt, wl.t_for, wt_out hold that many), W gains two count
    // columns, and the answers have their own page-locked block. !rpc(): not such a context.
    uint32_t n_wait_rows = 0;  // rows W's entries stand for after the last tick
    DevBuf<uint8_t> d_rpc;
    RpcEntryCols rw{}, rp{};   // W; the tick's positions [max_waiting | max_requests]
    RpcBatch rb{};
    RpcState* rs = nullptr;
    unsigned long long *lb_scan = nullptr, *lb_settle = nullptr, *lb_grant = nullptr;
    PinnedBuf h_rres;   // page-locked: the RpcOut sections
    RpcOut rh{}, rz{};  // ... at their host and device addresses
    // The running-task book B of a leased stream (ydc_stream_book_begin; running_book.h): its four
    // columns and its bookkeeping in HBM, its look-back words at the tail of `lookback`, the
    // page-locked outcome block. max_book == 0: no book (none of this exists). Sized by max_book,
    // except `staged`, which moves to a grown stream as it is.
    struct Book {
      uint32_t n = 0;  // |B| after the last tick (the outcome block's, kept here)
      DevBuf<uint8_t> d;
      BookCols bk{};
      BookState* bks = nullptr;
      unsigned long long* lb = nullptr;
      PinnedBuf h_res;  // page-locked: the outcome block
      BookOutcome *h_bout = nullptr, *z_bout = nullptr;
      // ydc_stream_book_stage: the payload columns of the next accepted tick's reports.
      struct Staged {
        bool on = false;
        std::vector<uint64_t> stid, dkey;
      } staged;
      // The digest index over B (book_index.h; ydc_stream_book_find / ydc_stream_book_distinct):
      // derived state, built on demand and sized by |B| then. `valid`: it describes B as B is now.
      // The rule errs on the stale side: a Book starts without an index (so every stream_alloc —
      // begin, end, ydc_stream_reserve, ydc_stream_book_begin, restore — drops it), and the two places
      // that launch a pass over B with something to drop clear the mark before the launch: a tick
      // that carries a report (stream_tick_stage) and remove_rows (ydc_remove_servants and the
      // removal route of a tick with aliveness). Everything else here is the read calls' scratch.
      struct Index {
        bool valid = false;
        DevBuf<uint8_t> d;  // key | last1 | cnt | side
        BookIndex ix{};
        DevBuf<unsigned long long> q;  // find: the queries ...
        DevBuf<BookHit> res;           // ... and their results
        DevBuf<uint8_t> rows;          // distinct: its state and look-back words | the five output columns
      } index;
    } book;
    // The servants' expiry column E of a leased stream (ydc_stream_alive_begin; servant_alive.h): sized
    // by the registry like d_rep_tick, with a spare the removal route compacts into. !alive.on: no
    // aliveness (none of this exists, and the step launches what it launches without it).
    struct Alive {
      bool on = false;
      uint32_t n = 0;  // rows of E that are filed (the registry's servant count, between ticks)
      DevBuf<int64_t> col, spare, d_stage;
      DevBuf<uint32_t> d_idx;
      DevBuf<AliveState> d_state;
      PinnedBuf due;  // page-locked: k_alive_due's list (uint32_t each)
      int64_t bound = INT64_MAX;  // <= min(E): only errs low; k_alive_due makes it exact
      uint64_t alarms = 0, removals = 0;  // ticks that launched k_alive_due; ... and removed rows
      // ydc_stream_alive_stage: the expiries of the next accepted tick's heartbeats.
      bool staged = false;
      std::vector<int64_t> stage;
      // What the most recent accepted tick erased (ydc_stream_alive_removed).
      std::vector<uint32_t> removed;
      uint32_t orphans = 0;
      OnceMarks once;  // over a tick's heartbeat list
      std::vector<uint32_t> rel, rep;  // the removal route's rewritten releases and report servants
    } alive;
    // Inspection (ydc_stream_inspect_begin; stream_inspect.h), beside the detail records above: the
    // servants' discovered_at / ever_assigned columns, sized by the registry like E, each with a spare
    // the removal route compacts into, and the read calls' scratch. !inspect.on: no inspection (none
    // of this exists, and the step launches what it launches without it).
    struct Inspect {
      bool on = false;
      uint32_t n = 0;  // rows of the two servant columns that are filed
      // The inspection epoch: counts the calls that rewrite records of leases that exist
      // already (ydc_stream_inspect_begin, ydc_stream_inspect_load); ydc_stream_inspect_restore adopts a
      // full sidecar's. A delta sidecar is applied only under the epoch it was taken in.
      uint64_t epoch = 0;
      DevBuf<int64_t> disc, disc_spare;
      DevBuf<unsigned long long> ever, ever_spare;
      DevBuf<uint32_t> avail;   // k_inspect_servants' per-servant result
      DevBuf<InspectSums> sums;
      DevBuf<uint8_t> pack;     // k_inspect_pack's columns and their count
    } inspect;
    // ydc_stream_inspect_select / ydc_stream_inspect_count (stream_select.h): the calls' scratch, grown
    // on demand: SelectState | the filters | k_select_pack's columns. Nothing a tick reads; a grown
    // stream starts without it. The filters go through a page-locked block of the stream's own, so
    // that their copy is an asynchronous one on the stream and not a blocking one out of the caller's memory.
    DevBuf<uint8_t> select;
    PinnedBuf select_h;
    // Withdrawal by tag (ydc_stream_withdraw_begin; stream_withdraw.h): the tick's list and counts in HBM
    // and the page-locked result block, sized by max_withdraw. max_withdraw == 0: none of this exists,
    // and the step launches what it launches without it. `host` moves to a grown stream as it is.
    struct Withdraw {
      DevBuf<uint8_t> d;  // tag | count | n
      WithdrawList list{};
      PinnedBuf h_res;  // page-locked: counts | WithdrawDone
      uint32_t *h_count = nullptr, *z_count = nullptr;
      WithdrawDone *h_done = nullptr, *z_done = nullptr;
      struct Host {
        // ydc_stream_withdraw_stage: the tags of the next accepted tick, as the caller gave them.
        bool staged = false;
        std::vector<uint64_t> tags;
        // The most recent accepted tick (ydc_stream_withdraw_result): per staged tag its place in the
        // tick's sorted list, the list's length, and the counts read back per place.
        std::vector<uint32_t> place, counts;
        uint32_t n_unique = 0;
      } host;
    } withdraw;
    // Departure of requestors (ydc_stream_depart_begin; stream_depart.h): the tick's list and counts in HBM
    // and the page-locked result block, sized by max_depart. max_depart == 0: none of this exists, and
    // the step launches what it launches without it. `host` moves to a grown stream as it is.
    struct Depart {
      DevBuf<uint8_t> d;  // ip | count | n
      DepartList list{};
      PinnedBuf h_res;  // page-locked: counts | DepartDone
      uint4 *h_count = nullptr, *z_count = nullptr;
      DepartDone *h_done = nullptr, *z_done = nullptr;
      struct Host {
        // ydc_stream_depart_stage: the requestors of the next accepted tick, as the caller gave them.
        bool staged = false;
        std::vector<uint32_t> ips;
        // The most recent accepted tick (ydc_stream_depart_result): the staged requestors, per staged
        // requestor its place in the tick's sorted list, and the counts read back per place.
        std::vector<uint32_t> asked, place;
        std::vector<uint4> counts;
        uint32_t n_unique = 0;
      } host;
    } depart;
    // The cap per requestor inside the tick (ydc_stream_quota_begin; stream_quota.h): the table keyed by
    // the tick's new requestors, the settings' device copy, the admitted counts per new request in HBM
    // and the page-locked results. !on: none of this exists, and the step launches what it launches
    // without it. `host` moves to a grown stream as it is.
    struct Quota {
      bool on = false;
      uint32_t max_overrides = 0;
      DevBuf<uint8_t> d;
      QuotaTable tb{};
      QuotaCaps caps{};
      QuotaTick tk{};
      uint32_t tiles = 0;
      PinnedBuf h_res;  // page-locked: admitted immediate | admitted prefetch | QuotaDone
      uint32_t *h_imm = nullptr, *z_imm = nullptr, *h_pre = nullptr, *z_pre = nullptr;
      QuotaDone *h_done = nullptr, *z_done = nullptr;
      // The fair-share level (ydc_stream_quota_fair; stream_fair.h): ask[] beside the table, the pairs of
      // fair askers, the sums, the tick's header and result and the settings' copy in HBM;
      // the page-locked result. They exist with the quota; a stream whose mode is off launches nothing on them.
      DevBuf<uint8_t> fd;
      FairTick fair{};
      PinnedBuf h_fair;
      FairResult *h_fres = nullptr, *z_fres = nullptr;
      struct Host {
        // ydc_stream_quota_set: the default and the overrides (sorted by requestor), and whether the
        // device copy still has to follow them (a set, a grown stream).
        uint32_t default_cap = YDC_QUOTA_UNLIMITED;
        std::vector<uint32_t> ip, cap;
        bool dirty = true;
        bool table_dirty = false;  // a tick ended in an error behind its clip: the table is cleared before the next
        // The most recent accepted tick (ydc_stream_quota_result).
        std::vector<uint32_t> imm, pre;
        uint32_t rows_clipped = 0, n_refused = 0;
        // ydc_stream_quota_fair: the mode and its two numbers (`dirty` covers them), and the most recent
        // accepted tick's result (ydc_stream_quota_fair_result).
        uint32_t fair_mode = kFairOff, fair_pool = 0, fair_floor = 0;
        FairResult fair_res{};
      } host;
      bool fair_on() const { return on && host.fair_mode != kFairOff; }
      // 0: off; otherwise max_overrides + 1 (what stream_alloc and stream_regrow are told).
      uint32_t code() const { return on ? max_overrides + 1 : 0; }
    } quota;
    // Usage per requestor (ydc_stream_usage_begin; stream_usage.h): the persistent table and its totals in
    // HBM, and a page-locked block of its own (the tick's dq | the result), so that no section of the
    // arena moves. !on: none of this exists, and the step launches what it launches without it. Keyed by
    // requestor and sized by its own keys, not by the stream's bounds: it moves to a grown stream as it is.
    struct Usage {
      bool on = false;
      int64_t quantum = 0;
      bool has_last = false;  // `last` is a clock (the begin call found a tick behind it, or a tick has run since)
      int64_t last = 0;
      DevBuf<uint8_t> d;  // word | the five sums
      DevBuf<UsageState> st;
      UsageTable tb{};
      PinnedBuf h;  // page-locked: dq | UsageDone
      unsigned long long *h_dq = nullptr, *z_dq = nullptr;
      UsageDone *h_done = nullptr, *z_done = nullptr;
      // The bound that errs high on the distinct keys the next accrual can meet: n_keys (exact: the
      // device's after the last tick, load or reset) + fresh (the keys L and W can have gained since an
      // accrual last claimed theirs: it adds up over ticks with dq == 0, which claim nothing; usage_bound).
      uint32_t n_keys = 0;
      uint64_t fresh = 0;
      // The read calls' and load's scratch.
      DevBuf<uint32_t> q;
      DevBuf<UsageRow> rows;
      DevBuf<uint8_t> fold;  // the fold's state and look-back words
      uint32_t slots() const { return on ? tb.mask + 1 : 0; }
    } usage;
    // ydc_stream_outlook_get (stream_outlook.h): scratch only, reserved at the first call and
    // released with the stream; nothing of it is state, so reserve / restore carry nothing over.
    struct Outlook {
      DevBuf<unsigned long long> agg, res;  // per class; per query (kOutlookCols each)
      DevBuf<uint32_t> q, hist;             // queries (env | minv); W's and L's histograms
    } outlook;
    // ydc_stream_requestor_find / _get (requestor_index.h): scratch only, like the outlook's. The index
    // is built by each call, so there is no mark to keep and nothing for reserve / restore to carry.
    struct Requestor {
      DevBuf<uint8_t> d;          // word | the five sums | unattributed
      DevBuf<uint32_t> q;         // find: the queries ...
      DevBuf<RequestorLoad> res;  // ... and their rows
      DevBuf<uint8_t> rows;       // get: the fold's state and look-back words | its rows
    } requestor;
    // ydc_stream_delta_base / ydc_stream_delta (stream_delta.h): the base a later delta is taken against.
    // On the device the packed image of L (two buffers: a delta scans into the other one and they
    // change roles when it succeeds), the lists' scratch and a copy of B's columns; on the host the
    // base's identity and the structure stamp. !on: no base. It lives and dies with this record, so
    // whatever replaces the stream (end, a begin call, restore, an effective ydc_stream_reserve or
    // *_begin of a capability) ends the chain. `apply`: ydc_stream_delta_apply's lists on the device.
    struct DeltaBase {
      bool on = false;
      DevBuf<uint8_t> img[2];  // id | expires_at | servant | state, `cap` records each
      uint32_t cur = 0, cap = 0, n = 0;
      DevBuf<uint8_t> lists;   // inserted (24 B) | erased (8 B) | updated (20 B), `cap` records each | DeltaCounts
      DevBuf<uint8_t> book;    // grant | stid | dkey | servant, max_book entries each
      uint32_t n_book = 0;
      unsigned long long next_id = 0;
      int64_t last_now = INT64_MIN;
      uint32_t lease_tick = 0, n_waiting = 0;
      uint64_t stamp = 0;
      DevBuf<uint8_t> apply;
    } delta;
  } stream_mode;
  // ydc_stream_snapshot: the packed columns of L with their count on the device, and the page-locked
  // block they cross the bus into. Kept for the next snapshot (a standby is fed periodically, and
  // the two allocations cost more than everything else the call does).
  DevBuf<uint8_t> d_snap;
  PinnedBuf h_snap;
  DevBuf<ClassRun> d_runs;
  DevBuf<uint8_t> d_dirty;
  bool debug_sim = false;
  DevBuf<DeviceParams> d_prm;
  PinnedAs<DeviceParams> h_prm;   // the outcome block: stored by k_finalize itself, or d_prm copied back
  bool opt_outcome_store = true;  // (outcome_store=0: always the copy)
  bool opt_requestor_combine = true;  // equal requestors combined inside the wave first (requestor_combine=0: an atomic per entry)
  bool opt_release_counted = true;  // long release lists counted in LDS first (release_counted=0: an atomic per slot)

  // Staging for the host-pointer entry point (ydc_dispatch): the three request columns in
  // one pinned arena and its device mirror (one H2D copy), the results (indexes |
  // running_tasks | utilisation) in another pair (one D2H copy, enqueued right behind the
  // finalise kernels so that the batch needs a single wait).
  // The request columns are only needed by the classification, so the slot generation and the
  // sort are enqueued first and run while the host stages the columns and the H2D copy travels on
  // a stream of its own (BatchCall::host_in, stage_host_requests).
  PinnedBuf h_in, h_res;  // (not mapped: they only feed and receive copies)
  PinnedAs<uint32_t> h_rel;  // staging of ydc_release_slots (not mapped either)
  OwnedEvent h_rel_ev;
  DevBuf<uint8_t> d_in, d_res;
  OwnedStream copy_stream;
  OwnedEvent copy_ev;
  DevBuf<uint32_t> d_out_idx, d_upd_idx;
  DevBuf<ydc_servant_row> d_upd_rows;

  // Small-batch path (tick_kernel.h): one launch per call, requests / deltas / results as kernel
  // arguments and plain stores to page-locked memory.
  DevBuf<uint32_t> d_ip;            // resident copy of the ip_id column (rebuild_tables)
  PinnedAs<TickDone> h_tick_done;  // page-locked, coherent: the kernel's stamp + counters
  PinnedBuf h_tick_io;             // page-locked arena: columns / deltas in, results out
  uint32_t tick_seq = 0;
  // Batches up to this many requests take it (small_batch=0: none does). kSmallBatchAuto: by
  // registry size — a pick costs ~1 us at 2k servants and ~4 us at 16k, the batch pipeline
  // ~90 / ~165 us whatever the batch holds (profiles/r05_td_latency_table.txt).
  static constexpr uint32_t kSmallBatchAuto = 0xFFFFFFFFu;
  uint32_t opt_small_batch = kSmallBatchAuto;
  // `same`: the requests are copies of one another (one RPC) and the kernel will place them as
  // one merge (tick_merges): ~0.5 us per request at 2k servants, ~1 us at 16k.
  uint32_t small_batch(bool same = false) const {
    if (opt_small_batch != kSmallBatchAuto) return opt_small_batch;
    return reg.n <= 4096 || same ? 64u : reg.n <= 8192 ? 48u : 32u;
  }
  uint64_t tick_batches = 0;
  // The resident form: the kernel of a COMMITting tick stays on its CU, the registry in its
  // registers, and takes the following ticks from a page-locked mailbox (tick_kernel.h: TickBox) —
  // no launch, no column loads. Every other use of the context ends it first (resident_stop).
  bool opt_resident = true;        // (resident=0: every tick is a launch)
  bool opt_tick_packed = true;     // (packed_tick=0: the two-word candidate everywhere)
  uint32_t opt_resident_idle_ms = 50;  // the kernel leaves by itself when nobody has asked for this long
  PinnedAs<TickBox> h_box;  // (the resident kernel reads it: resident_stop comes before its release)
  OwnedStream res_stream;
  OwnedEvent res_ev;
  bool res_live = false;  // a resident kernel was launched and has not been seen to leave
  bool res_util = false;  // ... and it stores utilisations (fixed at its launch: TickArgs::out_util)
  uint64_t tick_resident = 0, tick_launches = 0, pipeline_batches = 0;

  uint32_t opt_chunk_size = 0;     // 0: automatic
  uint32_t opt_target_chunks = 2048;
  // 16 KB of LDS per matching wave = 10 waves per CU. Smaller rings (more waves per CU, shorter
  // chunks) were measured and bring nothing: the waves saturate VALU issue at ~2 per SIMD. Nor do
  // rings sized to the class count help the batch on the other lane (NOTES_rejected.md 7.1).
  uint32_t opt_ring_total = 0;  // entries of a matching wave's rings; 0: chosen per batch (YDC_RING_TOTAL)
  uint32_t opt_bin_threads = 0;  // width of a k_bin_sort workgroup, 512 or 1024; 0: occupancy_plan.h's rule
  bool opt_group_walk = true;  // sparse eligibility: the walk in groups of 64 requests (YDC_GROUP_WALK=0: one at a time)
  uint32_t opt_zone_guess = 1;  // start guesses around the dedicated tier's end from a walk of that stretch: 1 where it pays, 2 always, 0 never
  // lead: where the walk starts, in levels before the tier's end (the first chunk boundary inside
  // it: up to a chunk less). It has to be on the true track when the transient begins (cfg3: 840
  // levels before the end; a start 1349 before it is too late, 1861 is not), and every request of
  // the lead delays the stretch's last chunk by 54 ns: the default, and more after a batch whose
  // served chunks did not come out consistent (zone_feedback).
  uint32_t opt_zone_lead = 2304, opt_zone_trail = 1024, opt_zone_max_chunks = 2560;
  uint32_t zone_lead_cur = 0;   // (0: opt_zone_lead) what zone_feedback has raised the lead to
  uint32_t zone_fails = 0, zone_cooldown = 0;  // failures at the largest lead; batches without a walk
  // Whether the walk pays is the registry's business (three of four seeds of cfg3's pool have no
  // chain at the tier's end: the chunks there would wait 200 us for cursors their level guesses
  // already had): decided from what batches of this shape cost on the device with and without it
  // (zone_decide / zone_feedback; zone_guess=2 forces the walk, 0 forbids it).
  struct ZoneArm {
    uint32_t n = 0;
    float ticks = 0;  // (moving average, 100 MHz)
  } zone_on, zone_off;
  uint32_t zone_off_rounds = 0;  // rounds of the last batch without the walk
  bool zone_cold = true;         // the shape's first batch has not been seen yet (not counted)
  uint32_t zone_since_probe = 0;
  uint64_t zone_shape = 0;       // the plans the figures above are about
  bool opt_walk_packed = true; // ... with head rank and class id in one word where they fit (walk_packed=0: two arrays)
  bool opt_fused_class = true;
  bool opt_own_guess = true;
  bool opt_pair = true;
  bool opt_packed_class = true;
  bool opt_shard_sort = true;
  // Bin sort (three launches, bin_sort.h) for registries that offer at most this many slots;
  // a batch with a bin too large for LDS is repeated with the radix sort, which then stays
  // (binsort_blocked) until the registry changes structure.
  bool opt_fuse_passes = true;  // one GPU: the launch of pass 0 does pass 1 as well (match_kernel.h)
  uint32_t opt_warm_up = 0;  // requests a chunk of pass 0 starts early (1 .. 64; 0: by chunk size)
  uint32_t opt_cp_every = 4;  // checkpoints before every 4th block of a chunk (MatchBuffers::cp_every)
  uint32_t opt_hand_tries = kHandTries;  // (tests: 0 makes most waves give up and leave their chunk to pass 2)
  bool opt_binsort = true;
  bool opt_stream_graph = true;  // the streaming step is replayed from its hipGraph (0: enqueued eagerly)
  bool opt_walk_park = true;  // k_walk_groups parks its fetches in a254 / a255 (0: in plain variables)
  bool opt_group_binsort = true;  // multi-GPU: bin sort of the whole registry before windowed radix (YDC_GROUP_BINSORT=0)
  bool opt_wide_lists = true;  // eligible-class lists for the wide kernel where every row is short (YDC_WIDE_LISTS=0: masks)
  bool opt_wide = true;  // > 256 classes: wave-per-chunk replay (YDC_WIDE=0: thread per chunk)
  uint32_t opt_binsort_max_slots = 600000;
  bool binsort_blocked = false;
  bool debug_verify_binsort = false;  // YDC_BINSORT_VERIFY=1: check every bin sort against a host sort
  uint64_t binsort_misses = 0;
  int64_t opt_shard_margin = -1;  // >= 0: margin of the key windows in slots (tests)
  uint32_t opt_rounds_per_check = 2;
  // Passes after which the matching stops repairing chunks in parallel and lets one wave walk
  // each chain to its end (match_kernel.h: walk): registries whose every chunk boundary carries a
  // state no guess predicts (a handful of servants with tens of thousands of slots and requests
  // from their own hosts: 554 passes, 1.2 s; healthy batches need 2 - 4) — `walk_after` passes, then
  // a scout and the walk.
  // COMMIT by exchanging the resident running_tasks column with k_finalize's output instead of
  // copying it back (BatchCall::by_swap).
  bool opt_commit_swap = true;  // (commit_swap=0: always the copy)
  uint32_t opt_walk_after = 12;
  uint32_t walked_at = 0;  // passes launched before the last batch's walk (0: it was not walked)
  bool profiling = false;
  OwnedEvent ev[YDC_STAGE_COUNT + 1];
  ydc_stats stats{};

  // Per-kernel timing (profiling only): one event pair per launch.
  struct KernelSample {
    const char* name;
    OwnedEvent a, b;
  };
  std::vector<KernelSample> ksamples;
  size_t ksamples_used = 0;
  std::string kprofile_json;
};

namespace {

// The six per-servant columns of the resident registry, listed once: the device column, where an
// upload (ydc_servant_soa), the host mirror and a snapshot hold it. d_spare[k] is the spare of
// kRegCols[k]. running_tasks has no host copy: it lives on the device alone.
struct RegCol {
  DevBuf<uint32_t> ydc_context::*dev;
  const uint32_t* ydc_servant_soa::*up;
  std::vector<uint32_t> RegistryMirror::*host;
  const uint8_t* snap::View::*snap;
};
constexpr RegCol kRegCols[6] = {
    {&ydc_context::d_version, &ydc_servant_soa::version, &RegistryMirror::version, &snap::View::version},
    {&ydc_context::d_nproc, &ydc_servant_soa::num_processors, &RegistryMirror::nproc, &snap::View::nproc},
    {&ydc_context::d_load, &ydc_servant_soa::current_load, &RegistryMirror::load, &snap::View::load},
    {&ydc_context::d_max_tasks, &ydc_servant_soa::max_tasks, &RegistryMirror::max_tasks, &snap::View::max_tasks},
    {&ydc_context::d_running, &ydc_servant_soa::running_tasks, nullptr, &snap::View::running},
    {&ydc_context::d_flags, &ydc_servant_soa::flags, &RegistryMirror::flags, &snap::View::flags}};

// What one batch is asked to do, handed down from the entry point to the launches: nothing of it
// is kept in the context.
struct BatchCall {
  uint32_t flags = 0;
  uint32_t* out_idx = nullptr;  // device addresses (NULL: not asked for)
  double* out_util = nullptr;
  uint32_t* out_running = nullptr;
  // ydc_dispatch from pageable memory: the request columns are staged and copied inside the batch,
  // behind the launches that do not read them (tk == NULL: they are on the device already).
  struct {
    const ydc_task_soa* tk = nullptr;
    uint32_t n = 0;
    size_t col = 0, bytes = 0;
  } host_in;
  // D2H copy to enqueue behind every finalise of the batch (bytes == 0: none).
  struct {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
  } post_copy;
  // The finalise: of a pipelined batch; where k_finalize hands the outcome to the host itself
  // (a device address; NULL: d_prm is read back with a copy — kernels.h: RunningArgs::host_outcome);
  // COMMIT by exchanging the running_tasks column with k_finalize's output afterwards, not by copy.
  bool pipelined = false;
  DeviceParams* outcome = nullptr;
  bool by_swap = false;
  // ydc_dispatch_wait placing a batch again after it has drained both lanes: a batch that is still
  // to be collected from the other lane is complete and not in the way.
  bool replay = false;
  bool staged() const { return host_in.tk || post_copy.bytes; }
};

// A batch outside a captured streaming step (which decides the last two for itself: the two
// addresses are baked into it). outcome: the page-locked block's device address.
BatchCall batch_call(const ydc_context* c, uint32_t flags, uint32_t* out_idx, double* out_util, uint32_t* out_running,
                     DeviceParams* outcome) {
  BatchCall b;
  b.flags = flags;
  b.out_idx = out_idx;
  b.out_util = out_util;
  b.out_running = out_running;
  // (k_finalize stores the outcome itself where it has servant workgroups)
  b.outcome = c->opt_outcome_store && c->reg.n ? outcome : nullptr;
  b.by_swap = c->opt_commit_swap && !c->stream_mode.active && (flags & YDC_DISPATCH_COMMIT) && c->reg.n;
  return b;
}

void stream_release(ydc_context* c);  // streaming mode, defined further down
int alive_fit(ydc_context* c);         // ... its servants' expiry column, defined further down
int inspect_fit(ydc_context* c, int64_t when);  // ... its inspection's servant columns, defined further down
void resident_stop(ydc_context* c);   // small-batch path's resident kernel, defined further down
void group_release(ydc_context* c);   // multi-GPU group, defined further down

// Errors raised before (or without) a context: process-wide, written from any thread.
std::mutex g_create_error_mu;
std::string g_create_error_text;
void set_create_error(std::string text) {
  std::lock_guard<std::mutex> lk(g_create_error_mu);
  g_create_error_text = std::move(text);
}
const char* create_error_cstr() {
  static thread_local std::string copy;  // (the caller reads it after the lock is gone)
  std::lock_guard<std::mutex> lk(g_create_error_mu);
  copy = g_create_error_text;
  return copy.c_str();
}

// Page-locked host ranges the device can address (ydc_host_register / ydc_host_alloc, or found
// pinned by the caller's own means): ydc_dispatch hands such buffers to the kernels as they are —
// request columns read and results written through the mapped pointer, no staging copy.
struct PinnedRange {
  const char* host;
  size_t bytes;
  char* dev;
  int kind;  // 0: registered here, 1: allocated here
};
std::mutex g_pinned_mu;
std::vector<PinnedRange> g_pinned;
// Pointers that were asked about and are NOT pinned (so that an unpinned caller does not pay a
// runtime query per batch); forgotten whenever a range is registered.
std::vector<const void*> g_not_pinned;

// Device address of [p, p + bytes) if it lies in a pinned range, else NULL.
void* pinned_device_pointer(const void* p, size_t bytes) {
  if (!p) return nullptr;
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  const char* q = (const char*)p;
  for (auto& r : g_pinned)
    if (q >= r.host && q + bytes <= r.host + r.bytes) return r.dev + (q - r.host);
  for (auto* np : g_not_pinned)
    if (np == p) return nullptr;
  // Pinned by the caller itself (hipHostMalloc / hipHostRegister outside this library)?
  // The whole range must lie in ONE pinned allocation: the last byte is asked about too and must
  // map where the first one's mapping continues (a column longer than its pinned part is staged).
  hipPointerAttribute_t a{}, z{};
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer) {
    if (bytes <= 1 ||
        (hipPointerGetAttributes(&z, q + bytes - 1) == hipSuccess && z.type == hipMemoryTypeHost &&
         z.devicePointer == (char*)a.devicePointer + (bytes - 1)))
      return a.devicePointer;  // (asked again next time: its owner may free it behind our back)
  }
  (void)hipGetLastError();
  if (g_not_pinned.size() >= 64) g_not_pinned.clear();
  g_not_pinned.push_back(p);
  return nullptr;
}

// Developer / test switchboard: ONE environment variable, YDC_TUNE="key=value,key=value", read
// when a context is created. It forces code paths the planner would not choose on its own (the
// parity tests cover the fallbacks with it: chunk and ring sizes, the radix pipeline on a
// registry the bin sort would take, the lone walker, ...).
// Not an interface: a scheduler never sets it, and nothing in it changes a placement.
const char* tune_value(const char* key) {
  static thread_local std::string value;
  const char* all = getenv("YDC_TUNE");
  if (!all) return nullptr;
  const size_t klen = std::strlen(key);
  for (const char* p = all; *p;) {
    const char* end = std::strchr(p, ',');
    const size_t len = end ? (size_t)(end - p) : std::strlen(p);
    if (len > klen && p[klen] == '=' && std::strncmp(p, key, klen) == 0) {
      value.assign(p + klen + 1, len - klen - 1);
      return value.c_str();
    }
    p += len + (end ? 1 : 0);
  }
  return nullptr;
}

int fail(ydc_context* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ctx->last_error = buf;
  }
  return code;
}

#define HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t e__ = (expr);                                                                 \
    if (e__ != hipSuccess)                                                                   \
      return fail(ctx, YDC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                  __FILE__, __LINE__);                                                       \
  } while (0)

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

int rebuild_tables(ydc_context* c) {
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  const RegistryMirror& reg = c->reg;
  const uint32_t n = reg.n;
  c->tables.build(n, reg.env.data(), reg.version.data(), reg.max_tasks.data(), reg.nproc.data(), reg.ip.data(),
                  reg.env_words, (uint32_t)reg.alias_ip.size(), reg.alias_ip.data(), reg.alias_servant.data());
  const uint32_t n_ip = (uint32_t)c->tables.ip_sorted.size();
  c->n_parts = c->tables.n_comp;
  const uint32_t C = c->tables.n_classes();
  // The class partition on the last key pass, which may be given room for it. Up to 8 classes:
  // with 30 (cfg4: 9 + 9 + (5 + 5) bits instead of 8 + 8 + 7 and a class pass) the three passes
  // took 188 us where the four take 155 — wider digits scatter worse, and the fused pass ranks
  // twice and writes a third array (profiles/r04: measured and rejected).
  uint32_t fuse_bits = 0;
  if (C > 1 && C <= kMaxFusedClasses && c->opt_fused_class)
    while ((1u << fuse_bits) < C) ++fuse_bits;
  c->kf = choose_key_format(c->tables.cap_bits, kMaxRadixBits, &c->n_parts, fuse_bits);
  if (C > 65535) return fail(c, YDC_ERR_TOO_MANY_CLASSES, "%u servant classes", C);
  HIP_TRY(c, c->d_class_of.reserve(n));
  HIP_TRY(c, c->d_ip.reserve(n));
  HIP_TRY(c, c->d_ip_sorted.reserve(n_ip));
  HIP_TRY(c, c->d_ip_servant.reserve(n_ip));
  HIP_TRY(c, c->d_ip_hash.reserve(c->tables.ip_hash.size()));
  HIP_TRY(c, hipMemcpyAsync(c->d_ip_hash.p, c->tables.ip_hash.data(), c->tables.ip_hash.size() * 4,
                            hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, c->d_bin_tile_start.reserve(c->tables.bin_tile_start.size()));
  HIP_TRY(c, c->d_bin_tile_base.reserve(c->tables.bin_tile_start.size()));
  HIP_TRY(c, hipMemcpyAsync(c->d_bin_tile_start.p, c->tables.bin_tile_start.data(),
                            c->tables.bin_tile_start.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, c->d_ip_filter.reserve(c->tables.ip_filter.size()));
  HIP_TRY(c, hipMemcpyAsync(c->d_ip_filter.p, c->tables.ip_filter.data(), c->tables.ip_filter.size() * 4,
                            hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, c->d_cls_env.reserve((size_t)C * c->reg.env_words));
  HIP_TRY(c, c->d_cls_ver.reserve(C));
  HIP_TRY(c, c->d_cls_begin.reserve(C + 1));
  HIP_TRY(c, c->d_part_base.reserve(kMaxComponents + 1));
  HIP_TRY(c, c->d_cls_single.reserve(C ? C : 1));
  if (C)
    HIP_TRY(c, hipMemcpyAsync(c->d_cls_single.p, c->tables.cls_single.data(), C, hipMemcpyHostToDevice,
                              c->stream));
  if (c->n_parts > 1) {
    HIP_TRY(c, c->d_cls_comp.reserve(C));
    HIP_TRY(c, hipMemcpyAsync(c->d_cls_comp.p, c->tables.cls_comp.data(), (size_t)C * 4,
                              hipMemcpyHostToDevice, c->stream));
  }
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(c->d_class_of.p, c->tables.class_of.data(), n * 4,
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ip.p, c->reg.ip.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ip_sorted.p, c->tables.ip_sorted.data(), (size_t)n_ip * 4,
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ip_servant.p, c->tables.ip_servant.data(), (size_t)n_ip * 4,
                              hipMemcpyHostToDevice, c->stream));
  }
  if (C) {
    HIP_TRY(c, hipMemcpyAsync(c->d_cls_env.p, c->tables.cls_env.data(), (size_t)C * c->reg.env_words * 8,
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_cls_ver.p, c->tables.cls_ver.data(), C * 4,
                              hipMemcpyHostToDevice, c->stream));
  }
  if (!c->tables.elig_off.empty()) {
    HIP_TRY(c, c->d_elig_off.reserve(c->tables.elig_off.size()));
    HIP_TRY(c, c->d_elig_cls.reserve(std::max<size_t>(c->tables.elig_cls.size(), 1)));
    HIP_TRY(c, hipMemcpyAsync(c->d_elig_off.p, c->tables.elig_off.data(), c->tables.elig_off.size() * 4,
                              hipMemcpyHostToDevice, c->stream));
    if (!c->tables.elig_cls.empty())
      HIP_TRY(c, hipMemcpyAsync(c->d_elig_cls.p, c->tables.elig_cls.data(), c->tables.elig_cls.size() * 4,
                                hipMemcpyHostToDevice, c->stream));
  }
  if (!c->tables.env_ver_mask.empty()) {
    HIP_TRY(c, c->d_ver_sorted.reserve(c->tables.ver_sorted.size()));
    HIP_TRY(c, c->d_env_ver_mask.reserve(c->tables.env_ver_mask.size()));
    HIP_TRY(c, hipMemcpyAsync(c->d_ver_sorted.p, c->tables.ver_sorted.data(),
                              c->tables.ver_sorted.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_env_ver_mask.p, c->tables.env_ver_mask.data(),
                              c->tables.env_ver_mask.size() * 8, hipMemcpyHostToDevice, c->stream));
  }
  // The host vectors are pageable: the copies above are complete on return only
  // after a sync (the tables may be rebuilt before the next launch otherwise).
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tables_dirty = false;
  c->binsort_blocked = false;   // another registry: the bins get another chance
  c->stream_mode.stale = true;  // a captured streaming step bakes the table sizes in
  return YDC_OK;
}

int reserve_registry(ydc_context* c, uint32_t n) {
  for (auto& col : kRegCols) HIP_TRY(c, (c->*col.dev).reserve(n));
  HIP_TRY(c, c->d_running_out.reserve(n));
  HIP_TRY(c, c->d_slot_base.reserve((size_t)n + 1));
  HIP_TRY(c, c->d_pos_last.reserve(n));
  return YDC_OK;
}

void mark(ydc_context* c, int stage) {
  if (c->profiling) (void)hipEventRecord(c->ev[stage], c->stream);
}

// ---- lanes (lane_rule.h; ydc_context::Lane) ----

// The one list of what belongs to a lane: f(the context's member, lane 1's).
template <typename F>
void lane_pairs(ydc_context* c, ydc_context::Lane& l, F f) {
  f(c->d_prm, l.d_prm);
  f(c->d_slot_base, l.d_slot_base), f(c->d_cls_begin, l.d_cls_begin), f(c->d_vals[0], l.d_vals[0]);
  f(c->d_vals[1], l.d_vals[1]), f(c->d_hist, l.d_hist), f(c->d_row_total, l.d_row_total);
  f(c->d_tile_first, l.d_tile_first), f(c->d_keys[0], l.d_keys[0]), f(c->d_keys[1], l.d_keys[1]);
  f(c->d_cls_by_g, l.d_cls_by_g), f(c->d_owner, l.d_owner), f(c->d_rank_to_g, l.d_rank_to_g);
  f(c->d_zone_box, l.d_zone_box), f(c->d_binbase, l.d_binbase), f(c->d_binruns, l.d_binruns);
  f(c->d_level_tab, l.d_level_tab), f(c->d_row_of, l.d_row_of), f(c->d_bin_tile_base, l.d_bin_tile_base);
  f(c->d_part_base, l.d_part_base), f(c->d_mask, l.d_mask), f(c->d_self_lo, l.d_self_lo);
  f(c->d_self_hi, l.d_self_hi), f(c->d_chunk_consuming, l.d_chunk_consuming), f(c->d_before, l.d_before);
  f(c->d_slot_of, l.d_slot_of), f(c->d_pos_last, l.d_pos_last), f(c->d_chunk_tail, l.d_chunk_tail);
  f(c->d_running_out, l.d_running_out), f(c->d_guess[0], l.d_guess[0]), f(c->d_endst, l.d_endst);
  f(c->d_checkpoint, l.d_checkpoint), f(c->d_early, l.d_early), f(c->d_claim, l.d_claim);
  f(c->d_hand, l.d_hand), f(c->d_runs, l.d_runs), f(c->d_dirty, l.d_dirty);
}

// Lane 1, made at its first batch, with what the context sizes outside plan_batch (by the registry
// and its tables: reserve_registry, rebuild_tables, ydc_create) as large as lane 0's. Everything
// else plan_batch reserves under the LaneScope, the zeroed stamp arrays included.
int lane1_prepare(ydc_context* c) {
  if (!c->lane1) {
    auto l = std::make_unique<ydc_context::Lane>();
    HIP_TRY(c, l->own.create());
    l->stream = l->own;
    HIP_TRY(c, l->d_prm.reserve(1));
    HIP_TRY(c, hipMemsetAsync(l->d_prm.p, 0, sizeof(DeviceParams), l->stream));  // batch_seq starts at 0
    c->lane1 = std::move(l);
  }
  ydc_context::Lane& l = *c->lane1;
  HIP_TRY(c, l.d_slot_base.reserve(c->d_slot_base.cap));
  HIP_TRY(c, l.d_pos_last.reserve(c->d_pos_last.cap));
  HIP_TRY(c, l.d_running_out.reserve(c->d_running_out.cap));
  HIP_TRY(c, l.d_cls_begin.reserve(c->d_cls_begin.cap));
  HIP_TRY(c, l.d_bin_tile_base.reserve(c->d_bin_tile_base.cap));
  HIP_TRY(c, l.d_part_base.reserve(c->d_part_base.cap));
  HIP_TRY(c, l.d_row_total.reserve(c->d_row_total.cap));
  return YDC_OK;
}

// For the length of one enqueue, lane `lane`'s stream, workspace and params are the context's
// current ones (lane 0: nothing to do, and nothing done).
struct LaneScope {
  ydc_context* c;
  bool on;
  static void exchange(ydc_context* c) {
    ydc_context::Lane& l = *c->lane1;
    std::swap(c->stream, l.stream);
    lane_pairs(c, l, [](auto& mine, auto& theirs) { std::swap(mine, theirs); });
  }
  LaneScope(ydc_context* ctx, uint32_t lane) : c(ctx), on(lane == 1) {
    if (on) exchange(c);
  }
  ~LaneScope() {
    if (on) exchange(c);
  }
  LaneScope(const LaneScope&) = delete;
  LaneScope& operator=(const LaneScope&) = delete;
};

bool lane1_busy(const ydc_context* c) {
  for (const auto& pd : c->pend)
    if (pd.active && !pd.rerun && pd.lb.lane == 1) return true;
  return false;
}

// First in every entry point that takes the context's stream to order it behind the outstanding
// batches (all but ydc_dispatch_device_async, ydc_dispatch_wait, ydc_get_stats, ydc_last_error):
// waits for lane 1 where it has a batch in flight. What follows may write what lane 1 reads, on the
// context's stream: the next batches stay on lane 0 until one of them has been seen complete.
void join_lanes(ydc_context* c) {
  ++c->lane0_epoch;
  if (c->lane1 && lane1_busy(c)) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->lane1->stream);
  }
}

// Brackets one kernel launch with events when profiling is on.
struct KernelTimer {
  ydc_context* c;
  ydc_context::KernelSample* s = nullptr;
  KernelTimer(ydc_context* ctx, const char* name) : c(ctx) {
    if (!c->profiling) return;
    if (c->ksamples_used == c->ksamples.size()) {
      ydc_context::KernelSample n{name, {}, {}};
      if (n.a.create() != hipSuccess || n.b.create() != hipSuccess) return;
      c->ksamples.push_back(std::move(n));
    }
    s = &c->ksamples[c->ksamples_used++];
    s->name = name;
    (void)hipEventRecord(s->a, c->stream);
  }
  ~KernelTimer() {
    if (s) (void)hipEventRecord(s->b, c->stream);
  }
};
#define YDC_LAUNCH(ctx, name, ...)            \
  do {                                        \
    KernelTimer kt__(ctx, name);              \
    hipLaunchKernelGGL(__VA_ARGS__);          \
  } while (0)

// pa (nullable): the chunk prefix rides in the histogram launch as one more workgroup.
template <typename KeyT>
int launch_sort_pass(ydc_context* c, const SortIn<KeyT>& in_, uint32_t n_tiles, void* out_keys,
                     bool out_u32, uint32_t* out_vals, const PrefixArgs* pa = nullptr,
                     bool have_hist = false) {
  SortIn<KeyT> in = in_;
  in.xcd_hist = 1;
  in.xcd_scatter = 0;  // (XCD-contiguous order there too was measured and rejected)
  in.dbg = 0;
  const uint32_t radix = 1u << in.bits;
  if (!have_hist)  // (the first pass's tile histograms come out of k_slot_gen)
    YDC_LAUNCH(c, "k_radix_hist", k_radix_hist<KeyT>, dim3(xcd_grid(n_tiles) + (pa ? 1 : 0)), dim3(kSortThreads),
               radix * 4, c->stream, in, c->d_prm.p, n_tiles, c->d_hist.p, pa ? *pa : PrefixArgs{});
  YDC_LAUNCH(c, "k_radix_scan", k_radix_scan, dim3(radix), dim3(256), 0, c->stream, n_tiles,
             c->d_hist.p, c->d_row_total.p);
  const size_t lds = (size_t)(kSortWaves + 1) * radix * 4;
  if (in.fused_cls_bits) {
    const size_t lds2 = lds + (size_t)(kSortWaves + 1) * (radix >> in.fused_cls_bits) * 4;
    YDC_LAUNCH(c, "k_radix_scatter", (k_radix_scatter_classed<KeyT>), dim3(xcd_grid(n_tiles)),
               dim3(kSortThreads), lds2, c->stream, in, c->d_prm.p, n_tiles, c->d_hist.p,
               c->d_row_total.p, (uint32_t*)out_keys, out_vals, c->d_rank_to_g.p);
  } else if (out_u32) {
    YDC_LAUNCH(c, "k_radix_scatter", (k_radix_scatter<KeyT, uint32_t>), dim3(xcd_grid(n_tiles)),
               dim3(kSortThreads), lds, c->stream, in, c->d_prm.p, n_tiles, c->d_hist.p,
               c->d_row_total.p, (uint32_t*)out_keys, out_vals);
  } else {
    YDC_LAUNCH(c, "k_radix_scatter", (k_radix_scatter<KeyT, uint64_t>), dim3(xcd_grid(n_tiles)),
               dim3(kSortThreads), lds, c->stream, in, c->d_prm.p, n_tiles, c->d_hist.p,
               c->d_row_total.p, (uint64_t*)out_keys, out_vals);
  }
  return YDC_OK;
}

}  // namespace

extern "C" {

const char* ydc_strerror(int code) {
  switch (code) {
    case YDC_OK: return "ok";
    case YDC_ERR_INVALID_ARGUMENT: return "invalid argument";
    case YDC_ERR_HIP: return "HIP runtime error";
    case YDC_ERR_NO_DEVICE: return "no usable gfx950 device (there is no CPU fallback)";
    case YDC_ERR_CAPACITY: return "capacity of the context exceeded";
    case YDC_ERR_TOO_MANY_CLASSES: return "too many servant classes";
    case YDC_ERR_NOT_CONVERGED: return "chunk states did not converge";
    case YDC_ERR_NO_BASE: return "no delta base (take a new ydc_stream_delta_base)";
    default: return "unknown error";
  }
}

const char* ydc_last_error(const ydc_context* ctx) {
  return ctx ? ctx->last_error.c_str() : create_error_cstr();
}

int ydc_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    set_create_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return 0;
  }
  return n;
}

int ydc_device_malloc(int device, size_t bytes, void** out) {
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return YDC_ERR_NO_DEVICE;
  hipError_t e = hipMalloc(out, bytes ? bytes : 1);
  if (e != hipSuccess) {
    set_create_error(std::string("hipMalloc: ") + hipGetErrorString(e));
    return YDC_ERR_HIP;
  }
  return YDC_OK;
}

int ydc_device_free(void* p) { return hipFree(p) == hipSuccess ? YDC_OK : YDC_ERR_HIP; }

int ydc_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? YDC_OK : YDC_ERR_HIP;
}

int ydc_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? YDC_OK : YDC_ERR_HIP;
}
uint32_t ydc_abi_version(void) { return YDC_ABI_VERSION; }

int ydc_create(int device, uint32_t max_servants, uint32_t max_tasks, uint32_t max_slots,
               void* stream, ydc_context** out) {
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // (a servant index is below the number of servants: with this bound none is ever a sentinel, of which
  // YDC_IDX_WITHDRAWN is the lowest; max_servants == 0 is bounded the same way where the registry grows)
  if (max_servants > YDC_IDX_WITHDRAWN) {
    set_create_error("max_servants " + std::to_string(max_servants) + " > " + std::to_string(YDC_IDX_WITHDRAWN));
    return YDC_ERR_INVALID_ARGUMENT;
  }
  int n_dev = 0;
  hipError_t de = hipGetDeviceCount(&n_dev);
  if (de != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) {
    set_create_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(de) + ", " +
                     std::to_string(n_dev) + " device(s), asked for " + std::to_string(device));
    return YDC_ERR_NO_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) return YDC_ERR_NO_DEVICE;
  auto* c = new ydc_context();
  c->device = device;
  c->max_servants = max_servants;
  c->max_tasks = max_tasks;
  c->max_slots = max_slots;
  if (stream) {
    c->stream = (hipStream_t)stream;
  } else {
    if (c->own_stream.create() != hipSuccess) {
      delete c;
      return YDC_ERR_HIP;
    }
    c->stream = c->own_stream;
  }
  if (c->d_prm.reserve(1) != hipSuccess || c->h_prm.reserve(sizeof(DeviceParams)) != hipSuccess ||
      c->d_row_total.reserve(1u << kMaxRadixBits) != hipSuccess) {
    ydc_destroy(c);
    return YDC_ERR_HIP;
  }
  (void)hipMemset(c->d_prm.p, 0, sizeof(DeviceParams));  // batch_seq starts at 0
  for (auto& e : c->ev) {
    if (e.create() != hipSuccess) {
      ydc_destroy(c);
      return YDC_ERR_HIP;
    }
  }
  if (const char* s = tune_value("debug_sim")) c->debug_sim = atoi(s) != 0;
  if (const char* s = tune_value("chunk_size")) c->opt_chunk_size = (uint32_t)atoi(s);
  if (const char* s = tune_value("target_chunks")) c->opt_target_chunks = (uint32_t)atoi(s);
  if (const char* s = tune_value("fused_class")) c->opt_fused_class = atoi(s) != 0;
  if (const char* s = tune_value("own_guess")) c->opt_own_guess = atoi(s) != 0;
  if (const char* s = tune_value("pair")) c->opt_pair = atoi(s) != 0;
  if (const char* s = tune_value("ring_total")) c->opt_ring_total = std::max(256u, (uint32_t)atoi(s));
  if (const char* s = tune_value("group_walk")) c->opt_group_walk = atoi(s) != 0;
  if (const char* s = tune_value("walk_packed")) c->opt_walk_packed = atoi(s) != 0;
  if (const char* s = tune_value("zone_guess")) c->opt_zone_guess = (uint32_t)std::max(0, atoi(s));
  if (const char* s = tune_value("zone_lead")) c->opt_zone_lead = (uint32_t)atoi(s);
  if (const char* s = tune_value("zone_trail")) c->opt_zone_trail = (uint32_t)atoi(s);
  if (const char* s = tune_value("zone_max_chunks")) c->opt_zone_max_chunks = (uint32_t)atoi(s);
  if (const char* s = tune_value("packed_class")) c->opt_packed_class = atoi(s) != 0;
  if (const char* s = tune_value("shard_sort")) c->opt_shard_sort = atoi(s) != 0;
  if (const char* s = tune_value("binsort")) c->opt_binsort = atoi(s) != 0;
  if (const char* s = tune_value("bin_threads")) c->opt_bin_threads = (uint32_t)std::max(0, atoi(s));
  if (const char* s = tune_value("stream_graph")) c->opt_stream_graph = atoi(s) != 0;
  if (const char* s = tune_value("walk_park")) c->opt_walk_park = atoi(s) != 0;
  if (const char* s = tune_value("fuse_passes")) c->opt_fuse_passes = atoi(s) != 0;
  if (const char* s = tune_value("warm_up")) c->opt_warm_up = (uint32_t)std::min(64, std::max(1, atoi(s)));
  if (const char* s = tune_value("hand_tries")) c->opt_hand_tries = (uint32_t)std::max(0, atoi(s));
  if (const char* s = tune_value("lanes")) c->opt_lanes = atoi(s) != 0;
  if (const char* s = tune_value("cp_every")) {
    uint32_t v = (uint32_t)std::max(1, atoi(s)), p2 = 1;
    while (p2 * 2 <= v && p2 < 1024) p2 *= 2;
    c->opt_cp_every = p2;
  }
  if (const char* s = tune_value("wide")) c->opt_wide = atoi(s) != 0;
  if (const char* s = tune_value("wide_lists")) c->opt_wide_lists = atoi(s) != 0;
  if (const char* s = tune_value("group_binsort")) c->opt_group_binsort = atoi(s) != 0;
  if (const char* s = tune_value("binsort_verify")) c->debug_verify_binsort = atoi(s) != 0;
  if (const char* s = tune_value("binsort_max_slots")) c->opt_binsort_max_slots = (uint32_t)atoll(s);
  if (const char* s = tune_value("shard_margin")) c->opt_shard_margin = atoll(s);
  if (const char* s = tune_value("small_batch")) c->opt_small_batch = (uint32_t)std::max(0ll, atoll(s));
  if (const char* s = tune_value("resident")) c->opt_resident = atoi(s) != 0;
  if (const char* s = tune_value("packed_tick")) c->opt_tick_packed = atoi(s) != 0;
  if (const char* s = tune_value("resident_idle_ms")) c->opt_resident_idle_ms = (uint32_t)std::max(1, atoi(s));
  if (const char* s = tune_value("commit_swap")) c->opt_commit_swap = atoi(s) != 0;
  if (const char* s = tune_value("outcome_store")) c->opt_outcome_store = atoi(s) != 0;
  if (const char* s = tune_value("release_counted")) c->opt_release_counted = atoi(s) != 0;
  if (const char* s = tune_value("requestor_combine")) c->opt_requestor_combine = atoi(s) != 0;
  if (const char* s = tune_value("walk_after")) c->opt_walk_after = (uint32_t)std::max(2, atoi(s));
  if (const char* s = tune_value("rounds_per_check"))
    c->opt_rounds_per_check = std::max(1, atoi(s));
  *out = c;
  return YDC_OK;
}

int ydc_destroy(ydc_context* c) {
  if (!c) return YDC_OK;
  (void)hipSetDevice(c->device);
  join_lanes(c);
  resident_stop(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  stream_release(c);
  group_release(c);
  // Everything else the context took goes with its members, in reverse order of declaration (the
  // device is current; the resident kernel, which reads h_box, has left).
  delete c;
  return YDC_OK;
}

int ydc_upload_servants(ydc_context* c, const ydc_servant_soa* sv, uint32_t n) {
  if (!c || (n && !sv)) return YDC_ERR_INVALID_ARGUMENT;
  if (sv && sv->env_words > YDC_MAX_ENV_WORDS)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "env_words %u > %u", sv->env_words, YDC_MAX_ENV_WORDS);
  if (n > (c->max_servants ? c->max_servants : YDC_IDX_WITHDRAWN))
    return fail(c, YDC_ERR_CAPACITY, "%u servants > max_servants %u", n, c->max_servants);
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (released slots may still be on their way)
  if (int rc = reserve_registry(c, n)) return rc;
  c->reg.assign(sv, n);  // (the aliases go too: they name rows of the table that is being replaced)
  if (n)
    for (auto& col : kRegCols)
      HIP_TRY(c, hipMemcpyAsync((c->*col.dev).p, sv->*col.up, n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return rebuild_tables(c);
}

int ydc_update_servants_wide(ydc_context* c, const uint32_t* idx, const ydc_servant_row* rows,
                             const uint64_t* env_masks, uint32_t env_words, uint32_t n) {
  if (!c || (n && (!idx || !rows))) return YDC_ERR_INVALID_ARGUMENT;
  if (env_masks && (env_words == 0 || env_words > YDC_MAX_ENV_WORDS))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "env_words %u out of range", env_words);
  // A row carries one mask word: on a wider table it would silently clear the servant's other
  // environments (KeepServantAlive replaces the whole set, task_dispatcher.cc:195-201).
  if (!env_masks && n && c->reg.env_words > 1)
    return fail(c, YDC_ERR_INVALID_ARGUMENT,
                "the table holds %u mask words per servant: use ydc_update_servants_wide", c->reg.env_words);
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  // Appends first (they may need bigger buffers).
  uint32_t new_n = c->reg.n;
  for (uint32_t i = 0; i < n; ++i) {
    if (idx[i] > new_n) return fail(c, YDC_ERR_INVALID_ARGUMENT, "servant index %u out of order", idx[i]);
    if (idx[i] == new_n) ++new_n;
  }
  if (new_n > (c->max_servants ? c->max_servants : YDC_IDX_WITHDRAWN))
    return fail(c, YDC_ERR_CAPACITY, "%u servants > max_servants %u", new_n, c->max_servants);
  if (env_masks && c->reg.widen_env(env_words)) c->tables_dirty = true;
  const uint32_t old_n = c->reg.n;
  if (new_n > c->d_version.cap) {
    // Grow: read the running column back, reallocate, re-upload everything. Released slots
    // (ydc_release_slots only enqueues) must have reached the column first.
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> run(old_n);
    if (old_n) HIP_TRY(c, hipMemcpy(run.data(), c->d_running.p, old_n * 4, hipMemcpyDeviceToHost));
    run.resize(new_n, 0);
    if (int rc = reserve_registry(c, std::max<uint32_t>(new_n, new_n + new_n / 2))) return rc;
    c->reg.resize(new_n);
    HIP_TRY(c, hipMemcpy(c->d_running.p, run.data(), new_n * 4, hipMemcpyHostToDevice));
    for (auto& col : kRegCols)
      if (col.host)
        HIP_TRY(c, hipMemcpy((c->*col.dev).p, (c->reg.*col.host).data(), new_n * 4, hipMemcpyHostToDevice));
  } else if (new_n > old_n) {
    c->reg.resize(new_n);
    HIP_TRY(c, hipMemsetAsync(c->d_running.p + old_n, 0, (new_n - old_n) * 4, c->stream));
  }
  bool structural = new_n != old_n;  // (the appended rows are there already, zeroed)
  for (uint32_t i = 0; i < n; ++i) {
    structural |= c->reg.structural(idx[i], rows[i], env_masks, env_words, i);
    c->reg.store_row(idx[i], rows[i], env_masks, env_words, i);
  }
  if (n) {
    // One staged copy of the update list + one scatter kernel (rows are SoA on the device).
    static_assert(sizeof(ydc_servant_row) == sizeof(ServantRowDev), "row layout");
    HIP_TRY(c, c->d_upd_idx.reserve(n));
    HIP_TRY(c, c->d_upd_rows.reserve(n));
    HIP_TRY(c, hipMemcpyAsync(c->d_upd_idx.p, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_upd_rows.p, rows, (size_t)n * sizeof(ydc_servant_row),
                              hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_apply_rows, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, c->d_upd_idx.p,
                       (const ServantRowDev*)c->d_upd_rows.p, n, c->reg.n, c->d_version.p,
                       c->d_nproc.p, c->d_load.p, c->d_max_tasks.p, c->d_flags.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (structural || c->tables_dirty) return rebuild_tables(c);
  return YDC_OK;
}

int ydc_update_servants(ydc_context* c, const uint32_t* idx, const ydc_servant_row* rows,
                        uint32_t n) {
  return ydc_update_servants_wide(c, idx, rows, nullptr, 1, n);
}

int ydc_set_host_aliases(ydc_context* c, const uint32_t* ip_id, const uint32_t* servant_idx, uint32_t n) {
  if (!c || (n && (!ip_id || !servant_idx))) return YDC_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; ++i)
    if (servant_idx[i] >= c->reg.n)
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "alias %u names servant %u of %u", i, servant_idx[i], c->reg.n);
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->reg.alias_ip.assign(ip_id, ip_id + n);  // (n == 0: none)
  c->reg.alias_servant.assign(servant_idx, servant_idx + n);
  return rebuild_tables(c);
}

// The body of ydc_remove_servants (idx: checked, ascending). in_tick: the removal route of a tick with
// aliveness on (servant_alive.h) — the leases of removed rows are parked for the tick's own steps
// instead of erased, and the host aliases of the survivors are kept and renumbered (the caller
// cannot set them again in the middle of a tick).
static int remove_rows(ydc_context* c, const uint32_t* idx, uint32_t n, bool in_tick) {
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  const uint32_t S = c->reg.n, kept = S - n;
  auto& sm = c->stream_mode;
  const bool leased = sm.active && sm.leased();
  const bool alive = leased && sm.alive.on;
  const bool inspect = leased && sm.inspect.on;
  // Everything that can fail for want of memory comes before the first launch: a removal is applied
  // to registry, leases, book and expiry column together or not at all.
  HIP_TRY(c, c->d_upd_idx.reserve(n));
  for (auto& b : c->d_spare) HIP_TRY(c, b.reserve(c->d_version.cap));
  if (alive) {
    if (int rc = alive_fit(c)) return rc;  // (rows the registry gained outside a tick: "never")
    HIP_TRY(c, sm.alive.spare.reserve(sm.alive.col.cap));
  }
  if (inspect) {
    // (rows the registry gained outside a tick: discovered at the last tick's clock)
    if (int rc = inspect_fit(c, sm.last_now == INT64_MIN ? 0 : sm.last_now)) return rc;
    HIP_TRY(c, sm.inspect.disc_spare.reserve(sm.inspect.disc.cap));
    HIP_TRY(c, sm.inspect.ever_spare.reserve(sm.inspect.ever.cap));
  }
  // Device: order-preserving compaction of the six resident columns into spare buffers,
  // which then take their place (running_tasks of the survivors never leaves the device).
  HIP_TRY(c, hipMemcpyAsync(c->d_upd_idx.p, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  CompactCols in{}, out{};
  for (int k = 0; k < 6; ++k) in.col[k] = (c->*kRegCols[k].dev).p, out.col[k] = c->d_spare[k].p;
  hipLaunchKernelGGL(k_compact_rows, dim3(ceil_div(S, 256)), dim3(256), 0, c->stream, in, out,
                     c->d_upd_idx.p, n, S);
  // A leased stream: the leases of the removed rows vanish (UnsafeSweepOrphans), the others follow
  // the compaction.
  if (leased && in_tick)
    hipLaunchKernelGGL(k_alive_remap, dim3(ceil_div(sm.lt.mask + 1, 256)), dim3(256), 0, c->stream, sm.lt,
                       c->d_upd_idx.p, n);
  else if (leased)
    hipLaunchKernelGGL(k_lease_remap, dim3(ceil_div(sm.lt.mask + 1, 256)), dim3(256), 0, c->stream, sm.lt, sm.ls,
                       c->d_upd_idx.p, n);
  // ... and with aliveness the expiry column follows the registry's columns.
  if (alive)
    hipLaunchKernelGGL(k_alive_compact, dim3(ceil_div(S, 256)), dim3(256), 0, c->stream, sm.alive.col.p,
                       sm.alive.spare.p, c->d_upd_idx.p, n, S);
  // ... and with inspection discovered_at and ever_assigned do.
  if (inspect)
    hipLaunchKernelGGL(k_inspect_compact, dim3(ceil_div(S, 256)), dim3(256), 0, c->stream, sm.inspect.disc.p,
                       sm.inspect.ever.p, sm.inspect.disc_spare.p, sm.inspect.ever_spare.p, c->d_upd_idx.p, n, S);
  // ... and with a running-task book the entries of the removed rows (DropServant).
  const bool booked = leased && sm.max_book;
  if (booked) {
    sm.book.index.valid = false;  // (positions and servant numbers move)
    const uint32_t tiles = ceil_div(sm.max_book, kBookTile);
    HIP_TRY(c, hipMemsetAsync(sm.book.lb, 0, (size_t)tiles * 8, c->stream));
    hipLaunchKernelGGL(k_book_remap, dim3(tiles), dim3(256), 0, c->stream, sm.book.bk, sm.book.bks, sm.max_book,
                       c->d_upd_idx.p, n, sm.book.lb);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (idx is pageable; the swap below retires the old columns)
  if (leased) HIP_TRY(c, hipMemcpy(&sm.n_leases, &sm.ls->n_leases, 4, hipMemcpyDeviceToHost));
  if (booked) HIP_TRY(c, hipMemcpy(&sm.book.n, &sm.book.bks->n_entries, 4, hipMemcpyDeviceToHost));
  for (int k = 0; k < 6; ++k) std::swap(c->*kRegCols[k].dev, c->d_spare[k]);
  if (alive) {
    std::swap(sm.alive.col, sm.alive.spare);
    sm.alive.n = kept;
  }
  if (inspect) {
    std::swap(sm.inspect.disc, sm.inspect.disc_spare);
    std::swap(sm.inspect.ever, sm.inspect.ever_spare);
    sm.inspect.n = kept;
    sm.stale = true;  // (a captured step holds the count column's address)
  }
  // Host mirror; in a tick the survivors' aliases stay, in the new numbering (elsewhere the caller
  // sets them again: row numbers moved).
  c->reg.compact(idx, n);
  if (in_tick) c->reg.renumber_aliases(idx, n);
  else c->reg.clear_aliases();
  return rebuild_tables(c);  // classes, the ip table and the slot bound follow the registry
}

int ydc_remove_servants(ydc_context* c, const uint32_t* idx, uint32_t n) {
  if (!c || (n && !idx)) return YDC_ERR_INVALID_ARGUMENT;
  if (!n) return YDC_OK;
  for (uint32_t i = 0; i < n; ++i)
    if (idx[i] >= c->reg.n || (i && idx[i] <= idx[i - 1]))
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "removed rows must be ascending and < %u", c->reg.n);
  return remove_rows(c, idx, n, false);
}

// FreeTask's --running_tasks for a list of grants (servant indexes on the device).
static void launch_release(ydc_context* c, const uint32_t* d_idx, uint32_t n) {
  if (n >= 4096 && c->reg.n <= 16384 && c->opt_release_counted) {
    if ((size_t)c->reg.n * 4 > 48 * 1024)  // (above 48 KB of dynamic LDS the runtime wants to be told)
      (void)hipFuncSetAttribute((const void*)k_release_slots_counted, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)c->reg.n * 4));
    hipLaunchKernelGGL(k_release_slots_counted, dim3(ceil_div(n, kReleaseTile)), dim3(1024),
                       (size_t)c->reg.n * 4, c->stream, d_idx, n, c->reg.n, c->d_running.p);
  } else {
    hipLaunchKernelGGL(k_release_slots, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, d_idx, n,
                       c->reg.n, c->d_running.p);
  }
}

int ydc_release_slots(ydc_context* c, const uint32_t* servant_idx, uint32_t n) {
  if (!c || (n && !servant_idx)) return YDC_ERR_INVALID_ARGUMENT;
  if (!n) return YDC_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, c->d_upd_idx.reserve(n));
  // Through a pinned staging buffer, stream-ordered: no wait here (the next batch follows on
  // the same stream). The buffer is reused only after its previous copy has run.
  if (c->h_rel_ev) HIP_TRY(c, hipEventSynchronize(c->h_rel_ev));
  if ((size_t)n * 4 > c->h_rel.cap)
    HIP_TRY(c, c->h_rel.reserve(std::max<size_t>((size_t)n * 6, 4096), hipHostMallocDefault));
  HIP_TRY(c, c->h_rel_ev.create(hipEventDisableTiming));
  std::memcpy(c->h_rel, servant_idx, (size_t)n * 4);
  HIP_TRY(c, hipMemcpyAsync(c->d_upd_idx.p, c->h_rel, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->h_rel_ev, c->stream));
  launch_release(c, c->d_upd_idx.p, n);
  HIP_TRY(c, hipGetLastError());
  return YDC_OK;
}

int ydc_release_slots_device(ydc_context* c, const uint32_t* d_servant_idx, uint32_t n) {
  if (!c || (n && !d_servant_idx)) return YDC_ERR_INVALID_ARGUMENT;
  if (!n) return YDC_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  launch_release(c, d_servant_idx, n);
  HIP_TRY(c, hipGetLastError());
  return YDC_OK;
}

int ydc_set_running(ydc_context* c, const uint32_t* running, uint32_t n) {
  if (!c || n != c->reg.n || (n && !running)) return YDC_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (released slots may still be on their way)
  if (n) HIP_TRY(c, hipMemcpy(c->d_running.p, running, n * 4, hipMemcpyHostToDevice));
  return YDC_OK;
}

int ydc_get_running(ydc_context* c, uint32_t* out, uint32_t n) {
  if (!c || n != c->reg.n || (n && !out)) return YDC_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (released slots may still be on their way)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n) HIP_TRY(c, hipMemcpy(out, c->d_running.p, n * 4, hipMemcpyDeviceToHost));
  return YDC_OK;
}

}  // extern "C" (reopened below)

// ---------------------------------------------------------------------------
// One batch = plan (sizes, workspace) + front (slots, sort, class lists, request
// classification, level guesses) + matching passes + finalise. The pieces only
// enqueue work on the context stream, so the streaming mode can capture them
// into a hipGraph; ydc_dispatch_device strings them together eagerly.
// ---------------------------------------------------------------------------
namespace {

// for_window: the plan of a multi-GPU batch whose slot sort is sharded (k_window generates only a
// key window of the slots: radix pipeline). beside: the batch may run next to one on the other
// lane (occupancy_plan.h).
bool zone_decide(ydc_context* c, uint32_t N, uint32_t K, uint32_t C);

int plan_batch(ydc_context* c, uint32_t N, BatchPlan* out, bool for_window = false, bool beside = false) {
  BatchPlan& p = *out;
  p = BatchPlan{};
  if (c->tables_dirty)
    if (int rc = rebuild_tables(c)) return rc;
  p.N = N;
  p.S = c->reg.n;
  p.C = c->tables.n_classes();
  p.W = std::max<uint32_t>(1, ceil_div(p.C, 64));
  const uint64_t slot_bound64 = c->tables.max_slots;
  if (slot_bound64 > 0xFFFFFFF0ull || (c->max_slots && slot_bound64 > c->max_slots))
    return fail(c, YDC_ERR_CAPACITY, "registry can offer %llu slots > max_slots %u",
                (unsigned long long)slot_bound64, c->max_slots);
  p.slot_bound = p.slot_bound_glob = (uint32_t)slot_bound64;
  // Sort tiles: 256 threads x `items` elements; fewer elements per thread while that still
  // leaves the chip short of workgroups (the passes are latency-bound at this size).
  p.sort_items = p.slot_bound <= 300000 ? 2 : (p.slot_bound <= 700000 ? 4 : 8);
  p.n_tiles = std::max<uint32_t>(1, ceil_div(p.slot_bound, kSortThreads * p.sort_items));
  p.any_shared = c->tables.any_shared_ip;
  p.use_generic = p.C > kMaxWaveClasses;
  p.wave_path = N && p.C && !p.use_generic;
  // A tuned size in whole blocks of 64 requests, like every automatic one: checkpoints are kept
  // per block ((kc * cs) >> 6 names a chunk's first), the chunks' tails are counted by the block
  // that ends them, and the walk of the tier's end steps through blocks and records its rows at
  // t_start + j * cs (zone_guess.h) — with 96 it would publish row j at another chunk's request.
  p.cs = (c->opt_chunk_size + 63u) & ~63u;
  if (p.cs == 0) {
    uint32_t want = ceil_div(std::max<uint32_t>(N, 1), std::max<uint32_t>(1, c->opt_target_chunks));
    p.cs = 64;
    while (p.cs < want && p.cs < 8192) p.cs <<= 1;
    // Big batches: twice the chunks while they stay at 1024 requests or more — four waves per
    // SIMD instead of two (cfg4, 4M requests: k_match_pass 373 -> 294 us). Shorter chunks cost
    // more in wrong guesses and replays than the occupancy brings (cfg3 at 256 instead of 512
    // requests per chunk: 395 -> 465 us).
    if (p.W == 1 && p.cs >= 2048) p.cs >>= 1;
  }
  // The many-class kernels replay whole chunks per round (no checkpoints): chunks long enough
  // for a wrong start to heal inside them keep the rounds few (cfg2 with 10 digests, 947 classes:
  // 16 / 10 / 6 / 4 rounds at 64 / 128 / 256 / 512 requests; 3.0 / 2.6 / 2.5 / 2.9 ms).
  if (p.use_generic && c->opt_chunk_size == 0) p.cs = std::max(p.cs, 256u);
  p.K = N ? ceil_div(N, p.cs) : 0;
  const uint32_t C = p.C, K = p.K, W = p.W, slot_bound = p.slot_bound;

  // Workspace.
  p.key32 = c->kf.key_bits <= 32;
  // 32-bit keys: 8-byte (key, value) records in d_keys; 64-bit keys: keys there, values in d_vals.
  HIP_TRY(c, c->d_keys[0].reserve(slot_bound));
  HIP_TRY(c, c->d_keys[1].reserve(slot_bound));
  if (!p.key32) {
    HIP_TRY(c, c->d_vals[0].reserve(slot_bound));
    HIP_TRY(c, c->d_vals[1].reserve(slot_bound));
  }
  p.packed = p.key32;
  HIP_TRY(c, c->d_hist.reserve(((size_t)1 << kMaxRadixBits) * p.n_tiles));
  HIP_TRY(c, c->d_tile_first.reserve((size_t)p.n_tiles + 2));
  if (C > 1) HIP_TRY(c, c->d_cls_by_g.reserve(slot_bound));
  p.key_passes = c->kf.passes;
  p.cls_passes = 0;
  p.fused_cls_bits = 0;
  p.gbits = 0;
  if (C > 1 && slot_bound) {
    uint32_t cls_bits = 1;
    while ((1u << cls_bits) < C) ++cls_bits;
    uint32_t gb = 1;
    while (gb < 32 && (slot_bound >> gb)) ++gb;
    if (gb + cls_bits <= 32 && c->opt_packed_class) p.gbits = gb;  // the class rides above the slot index
    // A handful of classes and room left in the last key digit: one pass does both.
    const uint32_t last_bits = c->kf.key_bits - (p.key_passes - 1) * c->kf.bits_per_pass;
    if (C <= kMaxFusedClasses && p.key_passes >= 1 && last_bits + cls_bits <= (uint32_t)kMaxRadixBits &&
        c->opt_fused_class) {
      p.fused_cls_bits = cls_bits;
      HIP_TRY(c, c->d_rank_to_g.reserve(slot_bound));
    } else {
      p.cls_passes = ceil_div(cls_bits, kMaxRadixBits);
      p.cls_bits = ceil_div(cls_bits, p.cls_passes);
    }
  }
  // Bin sort: 32-bit exact keys, the wave path's class limit, the class above the slot bits in
  // the value (or a single class), the whole slot order (a rank of a group takes it as well
  // unless it only sorts a key window). Decided from the registry alone.
  p.binsort = c->opt_binsort && !c->binsort_blocked && c->kf.exact && p.key32 && C >= 1 &&
              C <= kMaxWaveClasses && slot_bound && slot_bound <= c->opt_binsort_max_slots &&
              (C == 1 || p.gbits) && !for_window && p.S <= kBinMaxServants &&
              c->kf.cap_bits <= 11;
  if (p.binsort) {
    const BinFormat bf = choose_bins(c->kf.key_bits, slot_bound, kMaxBins);
    p.n_bins = bf.n_bins;
    p.bin_shift = bf.shift;
    // k_bin_sort keeps a record in one LDS word: key bits below the bin | slot | class.
    p.bin_slot_bits = 1;
    while (p.bin_slot_bits < 32 && (slot_bound >> p.bin_slot_bits)) ++p.bin_slot_bits;
    p.bin_cls_bits = 0;
    while ((1u << p.bin_cls_bits) < C) ++p.bin_cls_bits;
    // (more, narrower bins when the word is short of room for the key bits below the bin)
    while (p.bin_shift + p.bin_slot_bits + p.bin_cls_bits > 32 && p.n_bins < kMaxBins && p.bin_shift) {
      p.n_bins <<= 1;
      --p.bin_shift;
    }
    // Slot tiles: G consecutive servants, at most 2048 slots (a servant offers < 2^cap_bits).
    // (Smaller tiles were measured: more workgroups that each add up the servants before them
    // cost more than the fullest tile's shorter loop saves.)
    // Slot tiles: runs of consecutive servants cut by the host to about equal slot bounds
    // (host_tables.h: bin_tile_start; at most kBinMaxGroup servants and 2048 slots each).
    p.bin_group = kBinMaxGroup;
    p.bin_tiles = (uint32_t)c->tables.bin_tile_start.size() - 1;
    p.bin_threads = bin_sort_threads(c->opt_bin_threads, beside);
    if (p.bin_shift + p.bin_slot_bits + p.bin_cls_bits > 32 || p.bin_tiles > kBinMaxTiles) p.binsort = false;
  }
  if (p.binsort) {
    p.cls_passes = 0;
    p.fused_cls_bits = 0;
    HIP_TRY(c, c->d_binbase.reserve((size_t)(p.n_bins + 1) * (C + 1)));
    HIP_TRY(c, c->d_binruns.reserve((size_t)p.bin_tiles * p.n_bins));
    HIP_TRY(c, c->d_rank_to_g.reserve(slot_bound));
    HIP_TRY(c, c->d_level_tab.reserve(((size_t)(slot_bound >> 6) + 2) * C));
    // (consuming counts per wave of 64 requests instead of per chunk)
    HIP_TRY(c, c->d_chunk_consuming.reserve(((size_t)ceil_div(std::max(N, 1u), 64) + 1) * c->n_parts));
  }
  HIP_TRY(c, c->d_owner.reserve(slot_bound));
  HIP_TRY(c, c->d_mask.reserve((size_t)N * W));
  HIP_TRY(c, c->d_self_lo.reserve(N));
  HIP_TRY(c, c->d_self_hi.reserve(N));
  HIP_TRY(c, c->d_slot_of.reserve(N));
  HIP_TRY(c, c->d_chunk_consuming.reserve(((size_t)K + 1) * c->n_parts));
  HIP_TRY(c, c->d_before.reserve(((size_t)K + 2) * c->n_parts));
  HIP_TRY(c, c->d_dirty.reserve((size_t)K + 1));
  HIP_TRY(c, c->d_guess[0].reserve((size_t)K * C + 1));
  HIP_TRY(c, c->d_endst.reserve((size_t)K * C + 1));
  if (!p.use_generic) {
    HIP_TRY(c, c->d_checkpoint.reserve((size_t)ceil_div(std::max(N, 1u), 64) * C + 1));
    HIP_TRY(c, c->d_early.reserve((size_t)K * C + 1));
    if ((size_t)K + 1 > c->d_claim.cap) {
      // Claims compare against ever-growing (batch, pass) stamps: a fresh array starts at 0.
      HIP_TRY(c, c->d_claim.reserve((size_t)K + 1));
      HIP_TRY(c, hipMemsetAsync(c->d_claim.p, 0, c->d_claim.cap * 8, c->stream));
    }
  }
  if (p.use_generic && !(C <= kMaxWideClasses && c->opt_wide)) HIP_TRY(c, c->d_runs.reserve((size_t)K * C + 1));
  // Sparse eligibility (every (digest, version threshold) row names at most 64 classes): the wide
  // kernel reads a request's classes from its row instead of scanning C / 64 mask words.
  p.wide_lists = p.use_generic && C <= kMaxWideClasses && c->opt_wide && c->opt_wide_lists &&
                 !c->tables.elig_off.empty() && c->tables.elig_max_len <= 64;
  if (p.wide_lists) HIP_TRY(c, c->d_row_of.reserve(std::max(N, 1u)));

  p.sv = ServantTable{c->d_version.p, c->d_nproc.p,  c->d_load.p,     c->d_max_tasks.p,
                      c->d_running.p, c->d_flags.p, c->d_class_of.p, p.S};
  // The sort ping-pongs between the two key/value buffers: where the lists end up.
  const int cur = (int)(((slot_bound ? p.key_passes : 0) + p.cls_passes) & 1);
  const int key_sorted = (int)((slot_bound ? p.key_passes : 0) & 1);
  p.L.n_classes = C;
  p.L.cls_begin = c->d_cls_begin.p;
  p.L.cls_single = c->d_cls_single.p;
  if (p.packed) {
    const uint32_t* rec = (const uint32_t*)c->d_keys[cur].p;  // {rank, slot} pairs
    p.L.list_p = p.cls_passes || p.fused_cls_bits ? rec : nullptr;
    p.L.list_g = rec + 1;
    p.L.stride = 2;
    p.rank_to_g = p.fused_cls_bits ? c->d_rank_to_g.p : (const uint32_t*)c->d_keys[key_sorted].p + 1;
    p.rank_stride = p.fused_cls_bits ? 1 : 2;
  } else {
    p.L.list_p = p.cls_passes || p.fused_cls_bits ? (const uint32_t*)c->d_keys[cur].p : nullptr;
    p.L.list_g = c->d_vals[cur].p;
    p.L.stride = 1;
    p.rank_to_g = p.fused_cls_bits ? c->d_rank_to_g.p : c->d_vals[key_sorted].p;
    p.rank_stride = 1;
  }
  if (p.binsort) {
    // Staging records in d_keys[0], the class lists ({rank, slot} records) in d_keys[1].
    const uint32_t* rec = (const uint32_t*)c->d_keys[1].p;
    p.L.list_p = rec;
    p.L.list_g = rec + 1;
    p.L.stride = 2;
    p.rank_to_g = c->d_rank_to_g.p;
    p.rank_stride = 1;
  }
  p.T = TaskTable{c->d_mask.p, c->d_self_lo.p, c->d_self_hi.p, W};
  p.shared = SharedIpTable{c->d_ip_sorted.p, c->d_ip_servant.p, (uint32_t)c->tables.ip_sorted.size(),
                           c->d_class_of.p, c->d_slot_base.p, p.S, p.any_shared ? c->d_pos_last.p : nullptr};
  p.mb = MatchBuffers{};
  if (p.wave_path) {
    p.mb.guess0 = c->d_guess[0].p;
    p.mb.endst = c->d_endst.p;
    p.mb.checkpoint = c->d_checkpoint.p;
    // <= 64 classes on one GPU: pass 0 computes its level guesses itself (no k_guess_init).
    p.mb.before = p.W == 1 && c->group.n_ranks <= 1 && c->opt_own_guess ? c->d_before.p : nullptr;
    p.mb.cls_comp = c->d_cls_comp.p;
    p.mb.part_rank_base = c->d_part_base.p;
    p.mb.n_parts = c->n_parts;
    p.mb.early = c->d_early.p;
    p.mb.cp_every = c->opt_cp_every;
    p.mb.claim = c->d_claim.p;
    p.mb.slot_of = c->d_slot_of.p;
    p.mb.boundary_in = nullptr;
    p.mb.flags = c->d_prm.p->n_changed;
    p.mb.sampled = c->d_prm.p->n_sampled;
    p.mb.flag_mask = 63;
    p.mb.level_tab = p.binsort && c->n_parts <= 1 ? c->d_level_tab.p : nullptr;
    // The class partition as a pass of its own leaves its scanned histogram table in d_hist:
    // digit == class, one column per sort tile (enqueue_sort; k_radix_scan).
    if (!p.binsort && p.cls_passes == 1 && p.slot_bound) {
      p.mb.tile_tab = c->d_hist.p;
      p.mb.tile_tab_tiles = p.n_tiles;
      p.mb.tile_tab_elems = kSortThreads * p.sort_items;
    }
    // (a group of one rank is a single GPU with the exchanges of the protocol around it)
    p.fuse01 = c->opt_fuse_passes && c->group.n_ranks <= 1;
    if (p.fuse01) {
      if ((size_t)K * C * 4 > c->d_hand.cap) {
        // Granules are valid by their batch stamp (never 0): a fresh array starts at 0.
        HIP_TRY(c, c->d_hand.reserve((size_t)K * C * 4));
        HIP_TRY(c, hipMemsetAsync(c->d_hand.p, 0, c->d_hand.cap * 8, c->stream));
      }
      p.mb.hand = c->d_hand.p;
      p.mb.hand_tries = c->opt_hand_tries;
      HIP_TRY(c, c->d_chunk_tail.reserve((size_t)K + 1));
      p.mb.tail = c->n_parts <= 1 && p.mb.before ? c->d_chunk_tail.p : nullptr;
      // Warm-up length: an eighth of the chunk, 16 .. 64 requests (cfg2's chunks of 64: 16 is
      // enough for every chunk; cfg3's chunks of 512: 706 / 300 / 51 chunks still need a second
      // replay with 16 / 32 / 64, and the launch lasts as long as its slowest wave).
      p.mb.warm_len = c->opt_warm_up ? c->opt_warm_up : std::min(64u, std::max(kWarmUp, p.cs / 8));
    }
    // Ring of R = 2^rshift entries per class; a wave's rings hold 2048 entries in all
    // (16 KB of LDS: ranks + generation indexes), see match_kernel.h.
    p.ring_total = c->opt_ring_total;
    // The 4-waves-per-SIMD build of the matching kernel for chunks long enough to amortise its
    // spills (cfg2's chunks of 64 requests: 22.7 -> 23.1 us with it; cfg3's of 512: 426 -> 395),
    // and rings small enough for all of a CU's waves to be resident (160 KB of LDS, 16 waves).
    p.dense = p.W == 1 && p.cs >= 256;
    if (p.dense && c->opt_ring_total == 0) {
      const uint32_t per_cu = std::min<uint32_t>(16, std::max<uint32_t>(1, ceil_div(p.K, 256)));
      p.ring_total = 2048;
      while (p.ring_total > 256 && (size_t)per_cu * p.ring_total * 8 > 150 * 1024) p.ring_total >>= 1;
    } else if (c->opt_ring_total == 0) {
      p.ring_total = 2048;
    }
    while (p.ring_total < 2048 && ((size_t)C << 3) > p.ring_total) p.ring_total <<= 1;  // >= 8 per class
    p.rshift = 3;
    while (p.rshift < 10 && ((size_t)C << (p.rshift + 1)) <= p.ring_total) ++p.rshift;
    const uint32_t R = 1u << p.rshift;
    uint32_t want = 2 * p.cs / std::max(C, 1u);
    p.init_fill = 8;
    while (p.init_fill < want && p.init_fill < 64) p.init_fill <<= 1;
    p.init_fill = std::min(std::max(p.init_fill, 32u), R);
    // Few classes: the first fill is one coalesced load per class and 64 entries; take
    // enough for a whole block of 64 requests from one class.
    if (C <= 8) p.init_fill = std::min(128u, R);
    else if (C <= 16) p.init_fill = std::min(64u, R);
    // The stretch where the dedicated tier runs out, walked by one wave beside the first pass
    // (zone_guess.h: workgroup 0 of that launch). Where the passes are one round of
    // latency-bound waves — a chain behind the first launch then costs its full serial time
    // (cfg3: 224 of 384 us) —; a batch of more chunks hides its second replays behind the other
    // waves' work. (The walk's rings — ranks only, 128 entries per class at least — live in the
    // LDS a chunk's wave has.)
    p.zone = c->opt_zone_guess && p.W == 1 && p.mb.before && p.fuse01 && p.mb.tail && c->n_parts <= 1 &&
             !p.binsort && p.packed && c->kf.exact && p.key_passes >= 1 && C > 8 && C <= 64 && p.mb.tile_tab &&
             K >= 64 && K <= c->opt_zone_max_chunks && !for_window && slot_bound && !c->stream_mode.active &&
             ((size_t)C << 7) <= 2 * (size_t)p.ring_total;
    if (p.zone && c->zone_cooldown) {
      --c->zone_cooldown;
      p.zone = false;
    }
    p.zone_eligible = p.zone;
    if (p.zone && c->opt_zone_guess == 1) p.zone = zone_decide(c, N, K, C);
    if (p.zone) {
      const unsigned long long* had = c->d_zone_box.p;
      HIP_TRY(c, c->d_zone_box.reserve(2 + (size_t)kZoneMaxChunks * C));
      if (c->d_zone_box.p != had)  // (a granule is valid when it carries the batch's number: none does yet)
        HIP_TRY(c, hipMemsetAsync(c->d_zone_box.p, 0, c->d_zone_box.cap * 8, c->stream));
      p.mb.zone_box = c->d_zone_box.p;
      p.mb.zone_sorted = (const uint2*)c->d_keys[key_sorted].p;
      p.mb.zone_tier_shift = c->kf.key_bits - 1;
      p.mb.zone_lead = std::max(c->opt_zone_lead, c->zone_lead_cur);
      p.mb.zone_trail = c->opt_zone_trail;
    }
  }
  return YDC_OK;
}

// ---- the pieces of the front: servant scan | slot generation (+ request classification) |
// sort + class lists. enqueue_front_a strings them together; the multi-GPU path with a sharded
// sort puts its key-window selection between them (enqueue_front_windowed).

// Servant scan (also resets the per-batch device counters). cls_begin: where the class sizes
// of the whole registry go.
void enqueue_scan(ydc_context* c, const BatchPlan& p, uint32_t* cls_begin) {
  c->ksamples_used = 0;
  mark(c, 0);
  if (p.binsort) {  // (no scan: k_front_bins does without, see enqueue_gen)
    mark(c, 1);
    return;
  }
  // (one workgroup per slab of 1024 servants from 4k servants on: kernels.h, servant_scan_multi)
  const uint32_t scan_blocks = p.S > 4096 ? ceil_div(p.S, 1024) : 1u;
  YDC_LAUNCH(c, "k_servant_scan", k_servant_scan, dim3(scan_blocks), dim3(1024), (p.C + 1) * sizeof(uint32_t),
             c->stream, p.sv, p.C, p.slot_bound_glob, c->d_slot_base.p, cls_begin,
             c->d_chunk_consuming.p, p.K, PartTable{c->d_cls_comp.p, c->n_parts, c->d_part_base.p},
             kSortThreads * p.sort_items, p.win ? nullptr : c->d_tile_first.p, c->d_prm.p);
  mark(c, 1);
}

// Slot generation (one workgroup per sort tile: it leaves the tile's histogram of the first
// sort pass behind as well, kernels.h) and / or the request classification (class masks,
// own-servant ranges, consuming counts per chunk), which rides in the same launch as
// workgroups [gen_blocks, gen_blocks + cls_blocks).
void enqueue_gen(ydc_context* c, const BatchPlan& p, const ydc_task_soa* tk, bool gen, bool classify) {
  const uint32_t N = p.N, S = p.S, C = p.C, W = p.W, cs = p.cs;
  ClassifyArgs ca{};
  if (N && classify) {
    ca = ClassifyArgs{TaskColumns{tk->env_id, tk->min_version, tk->requestor_ip}, N,
                      c->d_cls_env.p, c->d_cls_ver.p, C, W, c->reg.env_words,
                      c->tables.env_ver_mask.empty() ? nullptr : c->d_ver_sorted.p,
                      c->tables.env_ver_mask.empty() ? nullptr : c->d_env_ver_mask.p,
                      (uint32_t)c->tables.ver_sorted.size(), c->d_ip_sorted.p, c->d_ip_servant.p, S,
                      c->d_slot_base.p, cs, c->d_mask.p, c->d_self_lo.p, c->d_self_hi.p,
                      c->d_chunk_consuming.p, c->d_cls_comp.p, c->n_parts,
                      p.mb.tail ? c->d_chunk_tail.p : nullptr, p.mb.warm_len,
                      p.binsort ? 1u : 0u, p.binsort ? 1u : 0u};
  }
  ca.n_ip = (uint32_t)c->tables.ip_sorted.size();
  ca.ip_hash = (const uint2*)c->d_ip_hash.p;
  ca.ip_hash_shift = c->tables.ip_hash_shift;
  ca.xcd_gen = 1;
  ca.ip_filter = c->d_ip_filter.p;
  ca.ip_filter_shift = c->tables.ip_filter_shift;
  ca.row_out = p.wide_lists && N && classify ? c->d_row_of.p : nullptr;
  ca.cls_comp = c->d_cls_comp.p;  // (k_slot_gen reads them for the part id above the key)
  ca.n_parts = c->n_parts;
  const uint32_t bpp0 = c->kf.bits_per_pass;
  const uint32_t fused0 = p.key_passes == 1 ? p.fused_cls_bits : 0;
  const uint32_t bits0 = std::min(bpp0, c->kf.key_bits) + fused0;
  const uint32_t gen_blocks = gen && p.slot_bound ? p.n_tiles : 0;
  // Large batches of the radix path: four requests per thread (kernels.h: task_classify_block_multi;
  // the lookup form with one mask word).
  ca.per_thread = classify && !p.binsort && N >= (1u << 18) && !c->tables.env_ver_mask.empty() && W == 1 &&
                          !ca.row_out ? 4u : 1u;
  const uint32_t cls_blocks = classify ? ceil_div(N, 256 * ca.per_thread) : 0;
  if (gen_blocks + cls_blocks == 0) return;
  const size_t lds0 = ((size_t)4 << bits0);
  // Key window (sharded sort): local prefix, first local slot and registry-wide names.
  const uint32_t* base = p.win ? c->group.ws.d_lbase.p : c->d_slot_base.p;
  const uint32_t* r_first = p.win ? c->group.ws.d_r_first.p : nullptr;
  const uint32_t* gbase = p.win ? c->d_slot_base.p : nullptr;
  uint16_t* cls_by_g = C > 1 && !p.gbits ? c->d_cls_by_g.p : nullptr;
  if (p.binsort && gen) {
    // Bin boundaries | slot tiles | requests: one launch, no workgroup waits for another.
    const BinTable bt{p.n_bins, p.bin_shift, c->d_binbase.p, c->d_binruns.p, p.bin_group, p.bin_tiles,
                      c->d_bin_tile_start.p, c->d_bin_tile_base.p};
    const size_t lds_words = std::max<size_t>((size_t)5 * p.n_bins + 7 * p.bin_group + 1, C + 1);
    YDC_LAUNCH(c, "k_front_bins", k_front_bins, dim3(p.n_bins + p.bin_tiles + cls_blocks), dim3(256),
               lds_words * 4, c->stream, p.sv, C, p.slot_bound_glob, c->d_slot_base.p, c->d_cls_begin.p,
               PartTable{c->d_cls_comp.p, c->n_parts, c->d_part_base.p}, c->d_prm.p, c->kf.cap_bits,
               c->kf.comp_shift, p.gbits, bt, c->d_owner.p, (uint2*)c->d_keys[0].p, ca);
    return;
  }
  const char* gen_name = gen_blocks && cls_blocks ? "k_slot_gen" : (gen_blocks ? "k_slot_gen(slots)" : "k_slot_gen(requests)");
  if (p.key32) {
    YDC_LAUNCH(c, gen_name, k_slot_gen<uint32_t>, dim3(xcd_grid(gen_blocks) + cls_blocks), dim3(256), lds0,
               c->stream, p.sv, base, c->d_prm.p, (uint32_t)c->kf.exact, c->kf.cap_bits,
               (uint32_t*)c->d_keys[0].p, c->d_vals[0].p, cls_by_g, c->d_owner.p,
               gen_blocks, p.sort_items, bits0, fused0, p.gbits, c->d_hist.p, ca, c->kf.comp_shift,
               r_first, gbase, p.packed ? 1u : 0u, p.win ? nullptr : c->d_tile_first.p);
  } else {
    YDC_LAUNCH(c, gen_name, k_slot_gen<uint64_t>, dim3(xcd_grid(gen_blocks) + cls_blocks), dim3(256), lds0,
               c->stream, p.sv, base, c->d_prm.p, (uint32_t)c->kf.exact, c->kf.cap_bits,
               (uint64_t*)c->d_keys[0].p, c->d_vals[0].p, cls_by_g, c->d_owner.p,
               gen_blocks, p.sort_items, bits0, fused0, p.gbits, c->d_hist.p, ca, c->kf.comp_shift,
               r_first, gbase, p.packed ? 1u : 0u, p.win ? nullptr : c->d_tile_first.p);
  }
}

// What the chunk prefix reads: counts per chunk, or (bin sort) per wave of 64 requests.
PrefixArgs prefix_args(ydc_context* c, const BatchPlan& p) {
  return PrefixArgs{c->d_chunk_consuming.p, p.K, c->d_before.p, c->n_parts,
                    p.binsort ? p.cs / 64 : 0u, p.binsort ? ceil_div(p.N, 64) : 0u};
}

// Sort by key + class lists. prefix_pending: the chunk prefix of the consuming counts still
// has to be computed — it goes with the first histogram launch (one more workgroup).
int enqueue_sort(ydc_context* c, const BatchPlan& p, bool prefix_pending) {
  const uint32_t N = p.N;
  void* keys[2] = {c->d_keys[0].p, c->d_keys[1].p};
  uint32_t* vals[2] = {c->d_vals[0].p, c->d_vals[1].p};
  int cur = 0;
  const PrefixArgs pa = prefix_args(c, p);
  const PrefixArgs* pending_prefix = N && prefix_pending ? &pa : nullptr;
  mark(c, 2);
  if (p.binsort) {
    // One workgroup per bin (+ one for the chunk prefix): order inside the bins, global ranks,
    // class lists.
    BinSortArgs ba{(const uint2*)c->d_keys[0].p,
                   BinTable{p.n_bins, p.bin_shift, c->d_binbase.p, c->d_binruns.p, p.bin_group, p.bin_tiles,
                            c->d_bin_tile_start.p, c->d_bin_tile_base.p},
                   p.C, p.gbits, p.bin_slot_bits, p.bin_cls_bits, c->d_slot_base.p, c->d_cls_begin.p,
                   (uint2*)c->d_keys[1].p, c->d_rank_to_g.p,
                   c->n_parts <= 1 ? c->d_level_tab.p : nullptr};
    // (the workgroup's width: occupancy_plan.h)
    const dim3 grid(p.n_bins + (pending_prefix ? 1 : 0));
    if (p.bin_threads == kBinThreadsNarrow) {
      YDC_LAUNCH(c, "k_bin_sort", k_bin_sort<kBinThreadsNarrow>, grid, dim3(kBinThreadsNarrow),
                 (size_t)BinShape<kBinThreadsNarrow>::kLdsWords * 4, c->stream, ba, c->d_prm.p,
                 pending_prefix ? pa : PrefixArgs{});
    } else {
      YDC_LAUNCH(c, "k_bin_sort", k_bin_sort<kBinThreadsWide>, grid, dim3(kBinThreadsWide),
                 (size_t)BinShape<kBinThreadsWide>::kLdsWords * 4, c->stream, ba, c->d_prm.p,
                 pending_prefix ? pa : PrefixArgs{});
    }
    mark(c, 3);
    mark(c, 4);
    return YDC_OK;
  }
  // ---- sort by key
  const uint32_t g_mask = p.gbits ? (1u << p.gbits) - 1 : 0xFFFFFFFFu;  // strips the class again
  const uint32_t bpp = c->kf.bits_per_pass;
  auto bits_of = [&](uint32_t q) { return std::min(bpp, c->kf.key_bits - q * bpp); };
  if (p.slot_bound) {
    for (uint32_t q = 0; q < p.key_passes; ++q) {
      // The last pass may carry the class above its key bits (k_radix_scatter_classed).
      const uint32_t fused = q + 1 == p.key_passes ? p.fused_cls_bits : 0;
      const uint16_t* cls = fused ? c->d_cls_by_g.p : nullptr;
      if (p.key32) {
        SortIn<uint32_t> in{(const uint32_t*)keys[cur], vals[cur], cls, q * bpp, bits_of(q) + fused,
                            p.sort_items, fused, p.gbits, fused ? g_mask : 0xFFFFFFFFu,
                            p.packed ? 1u : 0u, 0u};
        launch_sort_pass(c, in, p.n_tiles, keys[cur ^ 1], true, vals[cur ^ 1], q ? pending_prefix : nullptr,
                         q == 0);
      } else {
        SortIn<uint64_t> in{(const uint64_t*)keys[cur], vals[cur], cls, q * bpp, bits_of(q) + fused,
                            p.sort_items, fused, p.gbits, fused ? g_mask : 0xFFFFFFFFu, 0u, 0u};
        launch_sort_pass(c, in, p.n_tiles, keys[cur ^ 1], false, vals[cur ^ 1], q ? pending_prefix : nullptr,
                         q == 0);
      }
      if (q) pending_prefix = nullptr;
      cur ^= 1;
    }
  }
  mark(c, 3);
  // ---- class lists: stable partition of ranks by class
  for (uint32_t q = 0; q < p.cls_passes; ++q) {
    // First pass: key == index (global rank). Later passes carry the rank along.
    SortIn<uint32_t> in{q == 0 && !p.packed ? nullptr : (const uint32_t*)keys[cur], vals[cur],
                        c->d_cls_by_g.p, q * p.cls_bits, p.cls_bits, p.sort_items, 0u, p.gbits,
                        q + 1 == p.cls_passes ? g_mask : 0xFFFFFFFFu, p.packed ? 1u : 0u,
                        q == 0 ? 1u : 0u};
    launch_sort_pass(c, in, p.n_tiles, keys[cur ^ 1], true, vals[cur ^ 1], pending_prefix);
    pending_prefix = nullptr;
    cur ^= 1;
  }
  mark(c, 4);
  // Nothing was sorted (no free slot anywhere): the prefix gets a launch of its own.
  if (pending_prefix)
    YDC_LAUNCH(c, "k_chunk_prefix", k_chunk_prefix, dim3(1), dim3(1024), 0, c->stream, pa, c->d_prm.p);
  return YDC_OK;
}

// Everything before the level guesses: slots, sort, class lists, request classification.
int enqueue_front_a(ydc_context* c, const BatchPlan& p, const ydc_task_soa* tk) {
  enqueue_scan(c, p, c->d_cls_begin.p);
  enqueue_gen(c, p, tk, true, true);
  return enqueue_sort(c, p, true);
}

// Level guesses of the chunks' start states (base: consuming requests of earlier ranks,
// multi-GPU only) and the two special cases that bypass the matching passes.
int enqueue_front_b(ydc_context* c, const BatchPlan& p, const uint32_t* d_base) {
  const uint32_t N = p.N, S = p.S, C = p.C, K = p.K;
  DeviceParams* prm = c->d_prm.p;
  hipStream_t st = c->stream;
  if (N && C && !(p.wave_path && p.mb.before && !d_base))
    YDC_LAUNCH(c, "k_guess_init", k_guess_init, dim3(ceil_div(K * C, 256)), dim3(256), 0, st, p.L,
               c->d_before.p, K, d_base, PartTable{c->d_cls_comp.p, c->n_parts, c->d_part_base.p},
               c->d_guess[0].p, c->d_dirty.p);
  mark(c, 5);
  if (N && C == 0) {
    // No eligible servant at all: every request fails with EnvironmentNotFound
    // (task_dispatcher.cc:105-108).
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->d_slot_of.p, (int)kIdxEnvNotFound, N, st));
  }
  if (N && C && p.any_shared && p.slot_bound) {
    // Hosts that run several servants: the replays resolve `self` from the class state, which
    // takes the list position of every servant's last slot (dispatch_core.h: SharedIpTable).
    YDC_LAUNCH(c, "k_pos_last", k_pos_last, dim3(ceil_div(p.slot_bound, 256)), dim3(256), 0, st,
               p.L, c->d_owner.p, c->d_slot_base.p, prm, c->d_pos_last.p);
  }
  (void)S;
  return YDC_OK;
}

// Host columns -> pinned arena -> device mirror, on the copy stream; the dispatch stream waits
// for the copy (only the kernels behind this point read the columns).
int stage_host_requests(ydc_context* c, const BatchCall& call) {
  auto& h = call.host_in;
  std::memcpy(c->h_in.p, h.tk->env_id, (size_t)h.n * 4);
  std::memcpy(c->h_in.p + h.col, h.tk->min_version, (size_t)h.n * 4);
  std::memcpy(c->h_in.p + 2 * h.col, h.tk->requestor_ip, (size_t)h.n * 4);
  HIP_TRY(c, hipMemcpyAsync(c->d_in.p, c->h_in.p, h.bytes, hipMemcpyHostToDevice, c->copy_stream));
  HIP_TRY(c, hipEventRecord(c->copy_ev, c->copy_stream));
  HIP_TRY(c, hipStreamWaitEvent(c->stream, c->copy_ev, 0));
  return YDC_OK;
}

int enqueue_front(ydc_context* c, const BatchPlan& p, const ydc_task_soa* tk, const BatchCall& call) {
  if (call.host_in.tk && p.N) {
    // Host-buffer entry point: everything that does not read the requests first.
    enqueue_scan(c, p, c->d_cls_begin.p);
    enqueue_gen(c, p, tk, true, false);
    if (int rc = enqueue_sort(c, p, false)) return rc;
    if (int rc = stage_host_requests(c, call)) return rc;
    enqueue_gen(c, p, tk, false, true);
    const PrefixArgs pa = prefix_args(c, p);
    YDC_LAUNCH(c, "k_chunk_prefix", k_chunk_prefix, dim3(1), dim3(1024), 0, c->stream, pa, c->d_prm.p);
    return enqueue_front_b(c, p, nullptr);
  }
  if (int rc = enqueue_front_a(c, p, tk)) return rc;
  return enqueue_front_b(c, p, nullptr);
}

// One matching pass (match_kernel.h). device_check: return at once when the previous pass
// found every chunk consistent. walk: 8 for the walk's scout, 16 for the walk itself, 0 for an
// ordinary pass (match_kernel.h).
void enqueue_pass(ydc_context* c, const BatchPlan& p, uint32_t pass, uint32_t device_check, uint32_t walk = 0) {
  if (p.fuse01 && pass == 1) return;  // (the launch of pass 0 did it)
  const size_t lds = (size_t)p.ring_total * 8;
  device_check |= c->debug_sim ? 2u : 0u;
  device_check |= c->opt_pair ? 4u : 0u;
  device_check |= walk;
  device_check |= p.ring_total << 8;
  DeviceParams* prm = c->d_prm.p;
  // (rings of 32 entries are watched by the fast loop itself: match_kernel.h, CHECKED)
  const bool checked = p.W == 1 && p.rshift == 5;
  // (pass 0 of a plan with a zone walk: one workgroup more, the walk is the first — zone_guess.h)
  const uint32_t grid1 = p.K + (p.mb.zone_box && pass == 0 ? 1u : 0u);
#define YDC_LAUNCH_MATCH1(OCC, CHECKED)                                                             \
  YDC_LAUNCH(c, "k_match_pass", (k_match_pass<1, OCC, CHECKED>), dim3(grid1), dim3(64), lds, c->stream, \
             p.L, p.T, p.N, p.cs, p.K, p.mb, pass, device_check, p.rshift, p.init_fill, p.shared, prm)
  if (p.W == 1) {
    if (p.dense && checked) YDC_LAUNCH_MATCH1(4, true);
    else if (p.dense) YDC_LAUNCH_MATCH1(4, false);
    else if (checked) YDC_LAUNCH_MATCH1(1, true);
    else YDC_LAUNCH_MATCH1(1, false);
#undef YDC_LAUNCH_MATCH1
  } else if (p.W == 2) {
    YDC_LAUNCH(c, "k_match_pass", (k_match_pass<2>), dim3(p.K), dim3(64), lds, c->stream, p.L, p.T,
               p.N, p.cs, p.K, p.mb, pass, device_check, p.rshift, p.init_fill, p.shared, prm);
  } else {
    YDC_LAUNCH(c, "k_match_pass", (k_match_pass<4>), dim3(p.K), dim3(64), lds, c->stream, p.L, p.T,
               p.N, p.cs, p.K, p.mb, pass, device_check, p.rshift, p.init_fill, p.shared, prm);
  }
}

// slot -> servant index, utilisation, running_tasks (one launch). check_slot != kNone: only
// takes effect when the pass with that counter slot found every chunk consistent. start_state
// (multi-GPU): class states before this rank's first request; d_taken: its slot deltas.
int enqueue_finalize(ydc_context* c, const BatchPlan& p, const BatchCall& call, uint32_t check_slot,
                     uint32_t* d_taken = nullptr, const ClassState* start_state = nullptr) {
  const uint32_t S = p.S, N = p.N;
  const uint32_t req_blocks = ceil_div(N, 256), srv_blocks = ceil_div(S, 256);
  if (req_blocks + srv_blocks == 0) return YDC_OK;
  RunningArgs ra{};
  ra.end_state = N && p.C && p.K ? c->d_endst.p + (size_t)(p.K - 1) * p.C : nullptr;
  ra.start_state = ra.end_state ? start_state : nullptr;
  ra.L = p.L;
  ra.gslot_base = c->d_slot_base.p;
  ra.cls_comp = c->d_cls_comp.p;
  ra.n_parts = c->n_parts;
  ra.comp_shift = c->kf.comp_shift;
  ra.exact = c->kf.exact ? 1u : 0u;
  ra.cap_bits = c->kf.cap_bits;
  ra.n_servants = S;
  ra.running_out = c->d_running_out.p;
  ra.out_a = call.out_running;
  // The resident column is NOT written by this launch: its servant threads read the running
  // value of other servants (the head of their class list), so COMMIT is a copy behind it.
  ra.out_b = nullptr;
  ra.taken_out = d_taken;
  ra.pipelined = call.pipelined ? 1u : 0u;
  ra.host_outcome = srv_blocks && c->opt_outcome_store ? call.outcome : nullptr;
  ra.srv_blocks = srv_blocks;
  YDC_LAUNCH(c, "k_finalize", k_finalize, dim3(req_blocks + srv_blocks), dim3(256), 0, c->stream, p.sv,
             c->d_slot_base.p, c->d_owner.p, p.rank_to_g, c->d_slot_of.p, N, p.wave_path ? 1u : 0u,
             call.out_idx, call.out_util, check_slot, c->d_prm.p, p.gbits ? (1u << p.gbits) - 1 : 0xFFFFFFFFu,
             req_blocks, ra, p.rank_stride);
  // COMMIT (`++pick->running_tasks`, task_dispatcher.cc:123): running_out -> the resident column.
  // When the passes have not converged yet running_out == running and the step is repeated.
  // Round 5: no copy where the caller can simply make running_out THE column afterwards
  // (BatchCall::by_swap; a 4 us blit kernel per committed batch otherwise — kept where pointers are
  // baked into a captured step).
  if ((call.flags & YDC_DISPATCH_COMMIT) && S && !call.by_swap)
    HIP_TRY(c, hipMemcpyAsync(c->d_running.p, c->d_running_out.p, (size_t)S * 4, hipMemcpyDeviceToDevice,
                              c->stream));
  return YDC_OK;
}

// Internal return code: a bin of the bin sort did not fit its LDS buffer (bin_sort.h) — the
// batch was gated out on the device and is to be repeated with the radix sort.
constexpr int kRetryRadix = 1 << 20;

// Reads the batch counters back and decides: 1 converged (rounds set), 0 more passes needed,
// 2 the batch has to be repeated with the radix sort.
int read_outcome(ydc_context* c, const BatchPlan& p, uint32_t first, uint32_t launched,
                 uint32_t* rounds, bool stored_by_finalize = false) {
  if (!stored_by_finalize)
    HIP_TRY(c, hipMemcpyAsync(c->h_prm, c->d_prm.p, sizeof(DeviceParams), hipMemcpyDeviceToHost,
                              c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  if (c->h_prm->overflow)
    return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", p.slot_bound);
  if (p.binsort && c->h_prm->window_miss) return 2;
  if (c->h_prm->n_changed[(launched - 1) & 63] != 0) return 0;
  *rounds = launched;
  for (uint32_t r = first; r < launched; ++r)
    if (c->h_prm->n_changed[r & 63] == 0) {
      *rounds = r + 1;  // first pass that found nothing to do
      break;
    }
  return 1;
}

void fill_stats(ydc_context* c, const BatchPlan& p, uint32_t rounds) {
  ydc_stats& s = c->stats;
  std::memset(&s, 0, sizeof(s));
  ++c->pipeline_batches;
  s.n_tasks = p.N;
  s.n_servants = p.S;
  s.n_classes = p.C;
  s.n_slots = c->h_prm->n_slots;
  s.key_bits = c->kf.key_bits;
  s.radix_passes = p.binsort ? 0 : p.key_passes;  // 0: the bin sort placed the slots
  s.n_chunks = p.K;
  s.rounds = rounds;
  s.chunk_sims = c->h_prm->chunk_sims;
  // Every request is exactly one of: granted, Timeout (eligible classes exist but are full),
  // EnvironmentNotFound (no eligible class).
  s.granted = c->h_prm->granted;
  s.shard_sort_batches = (uint32_t)c->group.windowed_batches;
  s.shard_sort_misses = (uint32_t)c->group.window_misses;
  s.zone_rows = p.zone ? c->h_prm->zone_rows : 0u;
  s.env_not_found = p.N - std::min(p.N, c->h_prm->consuming);
  s.timeouts = p.N - s.env_not_found - std::min(p.N - s.env_not_found, s.granted);
}

// Per-kernel totals of the dispatch just finished as JSON: {"name": [launches, total_ms], ...}
// (profiling only: one event pair per YDC_LAUNCH).
void collect_kernel_profile(ydc_context* c) {
  std::vector<std::pair<std::string, std::pair<int, double>>> acc;
  for (size_t i = 0; i < c->ksamples_used; ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ksamples[i].a, c->ksamples[i].b) != hipSuccess) continue;
    bool found = false;
    for (auto& e : acc)
      if (e.first == c->ksamples[i].name) {
        e.second.first++;
        e.second.second += ms;
        found = true;
      }
    if (!found) acc.push_back({c->ksamples[i].name, {1, ms}});
  }
  std::string j = "{";
  for (size_t i = 0; i < acc.size(); ++i) {
    char buf[160];
    snprintf(buf, sizeof(buf), "%s\"%s\": [%d, %.6f]", i ? ", " : "", acc[i].first.c_str(),
             acc[i].second.first, acc[i].second.second);
    j += buf;
  }
  c->kprofile_json = j + "}";
}

// Walk or no walk for a batch of this shape? Without one until three batches (behind a first one
// that is not counted: cold caches) have shown a chain (more than two rounds); then three with it; then whichever costs less on the device
// (DeviceParams::t_begin .. t_end), the other one tried again every 64th batch.
bool zone_decide(ydc_context* c, uint32_t N, uint32_t K, uint32_t C) {
  const uint64_t shape = ((uint64_t)(N >> 12) << 40) | ((uint64_t)K << 16) | C;
  if (shape != c->zone_shape) {
    c->zone_shape = shape;
    c->zone_on = c->zone_off = ydc_context::ZoneArm{};
    c->zone_off_rounds = 0;
    c->zone_since_probe = 0;
    c->zone_cold = true;
  }
  if (c->zone_off.n < 3 || c->zone_off_rounds <= 2) return false;  // (no chain: nothing to cure)
  if (c->zone_on.n < 3) return true;
  const bool best = c->zone_on.ticks < c->zone_off.ticks;
  if (++c->zone_since_probe >= 64) {
    c->zone_since_probe = 0;
    return !best;
  }
  return best;
}

// After a batch with a zone walk (zone_guess.h): the chunks it served should have come out
// consistent in their first replay — two rounds. If not, the walk was not yet on the true track
// where the transient began: the next one starts earlier. (rows: DeviceParams::zone_rows.)
constexpr uint32_t kZoneLeadMax = 4096;
void zone_feedback(ydc_context* c, const BatchPlan& p, const DeviceParams& o, uint32_t rounds) {
  const uint32_t rows = o.zone_rows;
  if (p.zone_eligible) {
    const uint64_t t0 = ((uint64_t)o.t_begin_hi << 32) | o.t_begin_lo, t1 = ((uint64_t)o.t_end_hi << 32) | o.t_end_lo;
    ydc_context::ZoneArm& arm = p.zone ? c->zone_on : c->zone_off;
    if (c->zone_cold) {
      c->zone_cold = false;
    } else if (t1 > t0 && t1 - t0 < 100000000ull) {  // (stamped by this batch's first and last kernel)
      const float x = (float)(t1 - t0);
      arm.ticks = arm.n ? 0.75f * arm.ticks + 0.25f * x : x;
      ++arm.n;
    }
    if (!p.zone) c->zone_off_rounds = rounds;
  }
  if (!p.zone || rows < 2) return;
  if (rounds <= 2) {
    c->zone_fails = 0;
    return;
  }
  if (p.mb.zone_lead < kZoneLeadMax) {
    c->zone_lead_cur = std::min(p.mb.zone_lead + 512, kZoneLeadMax);
  } else if (++c->zone_fails >= 4) {  // this registry's transient is not one the walk tracks
    c->zone_fails = 0;
    c->zone_cooldown = 256;
  }
}

// Passes to launch before the first look at the outcome: what the last batch needed — and what
// the last batch WITHOUT the walk of the tier's end needed when this is one of those again
// (zone_decide tries the other arm now and then: it must not cost a pipeline miss).
uint32_t first_group(const ydc_context* c, const BatchPlan& p) {
  uint32_t hint = c->round_hint;
  if (p.zone_eligible && !p.zone) hint = std::max(hint, c->zone_off_rounds);
  return std::max(2u, std::min(hint, 16u));
}

// Passes [launched, ...) in groups until one finds every chunk consistent, each group
// followed by the (gated) finalise and one look at the counters.
int run_passes_until_consistent(ydc_context* c, const BatchPlan& p, uint32_t launched, const BatchCall& call,
                                uint32_t* rounds) {
  bool walked = false;
  for (;;) {
    const uint32_t group = launched == 0 ? first_group(c, p) : 4u;
    if (launched) {
      // Counter slots of the passes to come (the first group's were cleared by
      // k_servant_scan). The stream is idle here: the host has just synchronised.
      for (uint32_t r = launched; r < launched + group; ++r) {
        HIP_TRY(c, hipMemsetAsync(&c->d_prm.p->n_changed[r & 63], 0, 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(&c->d_prm.p->n_sampled[r & 63], 0, 4, c->stream));
      }
    }
    const uint32_t first = launched;
    if (launched >= c->opt_walk_after && !walked && group >= 4) {
      // Parallel repair is not getting anywhere (one chunk per pass): scout + walk, then two
      // ordinary passes that find everything consistent (match_kernel.h: walk_scout / walk_run).
      walked = true;
      c->walked_at = launched;
      HIP_TRY(c, hipMemsetAsync(&c->d_prm.p->reserved0, 0xFF, 4, c->stream));
      enqueue_pass(c, p, launched, 1u, 8u);
      enqueue_pass(c, p, launched + 1, 1u, 16u);
      for (uint32_t r = launched + 2; r < launched + group; ++r) enqueue_pass(c, p, r, 1u);
    } else {
      for (uint32_t r = launched; r < launched + group; ++r) enqueue_pass(c, p, r, 1u);
    }
    launched += group;
    if (int frc = enqueue_finalize(c, p, call, (launched - 1) & 63)) return frc;
    mark(c, 7);
    if (call.post_copy.bytes)  // a finalise that was gated out is repeated, and so is the copy
      HIP_TRY(c, hipMemcpyAsync(call.post_copy.dst, call.post_copy.src, call.post_copy.bytes,
                                hipMemcpyDeviceToHost, c->stream));
    int done = read_outcome(c, p, first, launched, rounds, call.outcome != nullptr);
    if (done < 0) return done;
    if (done == 2) return kRetryRadix;
    if (done) {
      // (the finalise just waited for was the final one: its output IS the column now)
      if (call.by_swap) std::swap(c->d_running, c->d_running_out);
      if (c->debug_sim) {
        fprintf(stderr, "[ydc match] K=%u cs=%u R=%u fill=%u rounds=%u sims=%u pass changed ends:", p.K,
                p.cs, 1u << p.rshift, p.init_fill, *rounds, c->h_prm->chunk_sims);
        for (uint32_t r = 0; r < *rounds; ++r) fprintf(stderr, " %u", c->h_prm->n_changed[r & 63]);
        fprintf(stderr, "\n");
      }
      return YDC_OK;
    }
    if (launched > p.K + 4)
      return fail(c, YDC_ERR_NOT_CONVERGED, "no fixpoint after %u passes", launched);
  }
}

// Debugging aid (YDC_BINSORT_VERIFY=1): the bin sort's outputs — global order, class lists —
// against a host sort of the very records k_front_bins staged. Waits for the stream.
int verify_binsort(ydc_context* c, const BatchPlan& p) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DeviceParams prm;
  HIP_TRY(c, hipMemcpy(&prm, c->d_prm.p, sizeof(prm), hipMemcpyDeviceToHost));
  const uint32_t M = prm.n_slots, C = p.C, row = C + 1;
  if (prm.window_miss) {
    fprintf(stderr, "[ydc binsort verify] a bin overflowed (window_miss): nothing to compare\n");
    return YDC_OK;
  }
  std::vector<uint2> stage(M), list(M);
  std::vector<uint32_t> r2g(M), cls_begin(C + 1), base((size_t)(p.n_bins + 1) * row);
  HIP_TRY(c, hipMemcpy(stage.data(), c->d_keys[0].p, (size_t)M * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(list.data(), c->d_keys[1].p, (size_t)M * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(r2g.data(), c->d_rank_to_g.p, (size_t)M * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(cls_begin.data(), c->d_cls_begin.p, (size_t)(C + 1) * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(base.data(), c->d_binbase.p, base.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t gmask = p.gbits ? (1u << p.gbits) - 1 : 0xFFFFFFFFu;
  uint32_t bad = 0, max_bin = 0;
  auto complain = [&](const char* what, uint32_t at, uint32_t got, uint32_t want) {
    if (++bad <= 12) fprintf(stderr, "[ydc binsort verify] %s at %u: device %u, host %u\n", what, at, got, want);
  };
  if (base[(size_t)p.n_bins * row + C] != M) complain("total of the last boundary row", p.n_bins, base[(size_t)p.n_bins * row + C], M);
  {
    // The closed-form bin starts against a count over the staged records (tile-major, any order).
    std::vector<uint32_t> cnt(p.n_bins + 1, 0);
    for (uint32_t i = 0; i < M; ++i) cnt[std::min(stage[i].x >> p.bin_shift, p.n_bins)]++;
    uint32_t acc = 0;
    for (uint32_t j = 0; j < p.n_bins; ++j) {
      if (base[(size_t)j * row + C] != acc) complain("start of bin", j, base[(size_t)j * row + C], acc);
      max_bin = std::max(max_bin, cnt[j]);
      acc += cnt[j];
    }
  }
  std::vector<uint2> sorted(stage);
  std::sort(sorted.begin(), sorted.end(), [&](const uint2& a, const uint2& b) {
    return a.x != b.x ? a.x < b.x : (a.y & gmask) < (b.y & gmask);
  });
  std::vector<uint32_t> next(cls_begin.begin(), cls_begin.end() - (C ? 1 : 0));
  for (uint32_t r = 0; r < M; ++r) {
    const uint32_t slot = sorted[r].y & gmask, cls = p.gbits ? sorted[r].y >> p.gbits : 0u;
    if (r2g[r] != slot) complain("rank_to_g", r, r2g[r], slot);
    if (cls < C) {
      const uint32_t at = next[cls]++;
      if (at < M && (list[at].x != r || list[at].y != slot)) {
        complain("class list rank", at, list[at].x, r);
        complain("class list slot", at, list[at].y, slot);
      }
    } else {
      complain("class of a record", r, cls, C);
    }
  }
  fprintf(stderr, "[ydc binsort verify] M=%u bins=%u shift=%u classes=%u fullest bin=%u: %u mismatches\n", M,
          p.n_bins, p.bin_shift, C, max_bin, bad);
  return bad ? fail(c, YDC_ERR_HIP, "bin sort verification failed (%u mismatches)", bad) : YDC_OK;
}

// Front, matching passes and finalise of a planned batch; returns when the results are there.
// kRetryRadix: the plan used the bin sort and a bin overflowed — nothing was committed.
int run_planned_batch(ydc_context* c, const BatchPlan& p, const ydc_task_soa* tk, const BatchCall& call,
                      uint32_t* rounds_out) {
  const uint32_t N = p.N;
  if (int rc = enqueue_front(c, p, tk, call)) return rc;
  if (p.binsort && c->debug_verify_binsort)
    if (int rc = verify_binsort(c, p)) return rc;
  hipStream_t st = c->stream;
  DeviceParams* prm = c->d_prm.p;
  uint32_t rounds = 0;
  mark(c, 6);
  if (p.wave_path) {
    c->walked_at = 0;
    if (int rc = run_passes_until_consistent(c, p, 0, call, &rounds)) return rc;
    // (a batch that had to be walked says nothing about how many passes the next one wants —
    // but if it is another of its kind, it should get to the walk as early)
    c->round_hint = c->walked_at ? std::min(c->walked_at, 3u) : rounds;
    zone_feedback(c, p, *c->h_prm, rounds);
  } else {
    if (N && p.C && p.use_generic) {
      // > kMaxWaveClasses classes: replay kernel + k_update per round, host-checked.
      const bool wide = p.C <= kMaxWideClasses && c->opt_wide;
      if (wide)  // (above 64 KB of dynamic LDS the runtime wants to be told)
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_sim_wide, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)wide_lds_bytes(kMaxWideClasses)));
      // The walk in groups of 64 requests (k_walk_groups) where the registry has eligible-class
      // lists and they fit the LDS beside the class states (YDC_GROUP_WALK=0: the lone walker).
      const uint32_t n_rows = p.wide_lists ? (uint32_t)c->tables.elig_off.size() - 1 : 0;
      const uint32_t n_list = p.wide_lists ? (uint32_t)c->tables.elig_cls.size() : 0;
      const bool group_walk = wide && p.wide_lists && c->opt_group_walk && p.C <= 65535 &&
                              group_walk_lds_bytes(p.C, n_rows, n_list) <= kGroupWalkMaxLds;
      // Head rank and class id in one word where both fit (and the extra array fits the LDS):
      // ranks are list positions of the whole registry here, below slot_bound.
      uint32_t walk_cbits = 1;
      while ((1u << walk_cbits) < p.C) ++walk_cbits;
      const bool walk_packed = group_walk && c->opt_walk_packed && c->group.n_ranks <= 1 &&
                               (uint64_t)p.slot_bound + 1 < ((uint64_t)1 << (32 - walk_cbits)) &&
                               group_walk_lds_bytes(p.C, n_rows, n_list, true) <= kGroupWalkMaxLds;
      if (group_walk)
        HIP_TRY(c, hipFuncSetAttribute(walk_packed ? (const void*)k_walk_groups<true> : (const void*)k_walk_groups<false>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGroupWalkMaxLds));
      uint32_t last_changed = 0xFFFFFFFFu;
      bool walked = false;
      if (group_walk) {
        // Sparse eligibility (eligible-class lists): no level to guess from, so no rounds of
        // speculation at all — the batch is walked from its first request, 64 requests at a time
        // (chunk 0's start state is the true one, k_guess_init; every chunk is still marked).
        if (walk_packed)
          YDC_LAUNCH(c, "k_walk_groups", k_walk_groups<true>, dim3(1), dim3(64),
                     group_walk_lds_bytes(p.C, n_rows, n_list, true), st, p.L, p.T, N, p.cs, p.K, c->d_guess[0].p,
                     c->d_endst.p, c->d_dirty.p, c->d_slot_of.p, p.shared, rounds, prm,
                     WideLists{c->d_row_of.p, c->d_elig_off.p, c->d_elig_cls.p}, n_rows, n_list, 1u, walk_cbits,
                     c->opt_walk_park ? 0u : 1u);
        else
          YDC_LAUNCH(c, "k_walk_groups", k_walk_groups<false>, dim3(1), dim3(64),
                     group_walk_lds_bytes(p.C, n_rows, n_list), st, p.L, p.T, N, p.cs, p.K, c->d_guess[0].p,
                     c->d_endst.p, c->d_dirty.p, c->d_slot_of.p, p.shared, rounds, prm,
                     WideLists{c->d_row_of.p, c->d_elig_off.p, c->d_elig_cls.p}, n_rows, n_list, 1u, walk_cbits,
                     c->opt_walk_park ? 0u : 1u);
        ++rounds;
        HIP_TRY(c, hipMemcpyAsync(c->h_prm, prm, sizeof(DeviceParams), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->h_prm->overflow)
          return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", p.slot_bound);
      }
      for (; !group_walk;) {
        for (uint32_t b = 0; b < c->opt_rounds_per_check; ++b) {
          ClassState* gold = c->d_guess[0].p;
          if (wide) {
            // One wave per chunk, the class states in LDS (wide_kernel.h) — or, once the rounds
            // have stopped making headway, one wave that walks the rest of the batch.
            const bool walk = walked;
            YDC_LAUNCH(c, walk ? "k_sim_wide(walk)" : "k_sim_wide", k_sim_wide, dim3(walk ? 1u : p.K),
                       dim3(64), wide_lds_bytes(p.C), st, p.L, p.T, N, p.cs, p.K, gold,
                       c->d_endst.p, c->d_dirty.p, c->d_slot_of.p, p.shared, rounds, prm, walk ? 1u : 0u,
                       p.wide_lists ? WideLists{c->d_row_of.p, c->d_elig_off.p, c->d_elig_cls.p}
                                    : WideLists{nullptr, nullptr, nullptr});
          } else {
            YDC_LAUNCH(c, "k_sim_generic", k_sim_generic, dim3(ceil_div(p.K, 64)), dim3(64), 0, st, p.L,
                       p.T, N, p.cs, p.K, gold, c->d_endst.p, c->d_dirty.p, c->d_slot_of.p, c->d_runs.p,
                       p.shared, rounds, prm);
          }
          YDC_LAUNCH(c, "k_update", k_update, dim3(std::max(1u, ceil_div(p.K * p.C, 256))), dim3(256),
                     0, st, p.C, p.K, c->d_endst.p, gold, c->d_dirty.p, rounds, prm);
          ++rounds;
        }
        HIP_TRY(c, hipMemcpyAsync(c->h_prm, prm, sizeof(DeviceParams), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->h_prm->overflow)
          return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", p.slot_bound);
        const uint32_t changed = c->h_prm->n_changed[(rounds - 1) & 63];
        if (changed == 0) break;
        if (walked) return fail(c, YDC_ERR_NOT_CONVERGED, "the walk left %u inconsistent states", changed);
        // Guesses that are still changing almost as much as a check ago: corrections are
        // travelling chunk by chunk. Stop speculating.
        if (wide && rounds >= 4 && changed > last_changed / 4 * 3) walked = true;
        last_changed = changed;
        if (rounds > p.K + 4)
          return fail(c, YDC_ERR_NOT_CONVERGED, "no fixpoint after %u rounds", rounds);
      }
    }
    BatchCall fin = call;
    fin.outcome = nullptr;  // (the host has checked the rounds itself: d_prm is read back below)
    if (int frc = enqueue_finalize(c, p, fin, kNone)) return frc;
    mark(c, 7);
    if (call.post_copy.bytes)
      HIP_TRY(c, hipMemcpyAsync(call.post_copy.dst, call.post_copy.src, call.post_copy.bytes,
                                hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(c->h_prm, prm, sizeof(DeviceParams), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipGetLastError());
    if (c->h_prm->overflow)
      return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", p.slot_bound);
    if (p.binsort && c->h_prm->window_miss) return kRetryRadix;
    if (call.by_swap) std::swap(c->d_running, c->d_running_out);  // (an ungated finalise: always final here)
  }
  *rounds_out = rounds;
  return YDC_OK;
}

// A bin of the bin sort overflowed: from now on (until the registry changes structure) the
// radix sort — batches planned after this take it.
void note_bin_overflow(ydc_context* c) {
  c->binsort_blocked = true;
  ++c->binsort_misses;
  c->stream_mode.stale = true;
}

// Plans a batch and places it, host-checked (*p: the plan it was placed with); a bin overflow
// places it once more with the radix sort.
int place_batch(ydc_context* c, uint32_t N, const ydc_task_soa* tk, const BatchCall& call, BatchPlan* p,
                uint32_t* rounds_out) {
  if (int rc = plan_batch(c, N, p)) return rc;
  int rc = run_planned_batch(c, *p, tk, call, rounds_out);
  if (rc == kRetryRadix) {
    note_bin_overflow(c);
    if (int rc2 = plan_batch(c, N, p)) return rc2;
    rc = run_planned_batch(c, *p, tk, call, rounds_out);
  }
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------------
// The small-batch path (tick_kernel.h): a handful of requests, the heartbeat rows that change no
// structure and the released grants that came in since the last call — one launch, no copy
// command; the host spins on the stamp the kernel stores last.
// ---------------------------------------------------------------------------
namespace {

// Registries and batches the one-workgroup kernel takes (tables must be current).
// The one-word candidate where the integer key and a registry index share 32 bits (capacities
// below 2^10 and a registry that leaves room: every realistic pool); the reference's double as
// the key otherwise (packed_tick=0: always).
bool tick_packed(const ydc_context* c, uint32_t* idx_bits_out = nullptr) {
  uint32_t idx_bits = 1;
  while ((1u << idx_bits) < std::max(c->reg.n, 2u)) ++idx_bits;
  if (idx_bits_out) *idx_bits_out = idx_bits;
  return c->opt_tick_packed && c->tables.cap_bits <= 10 && 2 * c->tables.cap_bits + 1 + idx_bits <= 32;
}

// Host request columns that are copies of their first entry (what one RPC sends).
bool tick_same_requests(const ydc_task_soa* tk, uint32_t n) {
  if (!tk || n < 2 || n > kTickBlock) return false;
  const uint32_t *e = (const uint32_t*)tk->env_id, *m = (const uint32_t*)tk->min_version,
                 *r = (const uint32_t*)tk->requestor_ip;
  for (uint32_t i = 1; i < n; ++i)
    if (e[i] != e[0] || m[i] != m[0] || r[i] != r[0]) return false;
  return true;
}

bool tick_takes(const ydc_context* c, uint32_t n_tasks, bool same = false) {
  same = same && tick_packed(c);  // (the wide builds of the kernel merge with one-word candidates only)
  return n_tasks <= c->small_batch(same) && c->small_batch() && c->reg.n <= kTickMaxServants &&
         c->tables.n_classes() <= kTickMaxClasses && c->reg.alias_ip.empty() && c->group.n_ranks == 0 &&
         !c->stream_mode.active && c->pend_count == 0 && !c->debug_sim && !c->debug_verify_binsort;
}

// ---- the resident kernel (tick_kernel.h: TickBox) ----
// Contexts whose resident kernel may still be polling its mailbox: told to leave when the process
// exits without destroying them (the kernel reads page-locked memory the runtime is about to unmap).
std::mutex g_resident_mu;
std::vector<ydc_context*> g_resident;
bool g_resident_atexit = false;

inline unsigned long long box_load(const unsigned long long* p) {
  return __atomic_load_n(p, __ATOMIC_ACQUIRE);
}

// Waits until granule `g` of the reply carries command number `seq`; false when the kernel has left
// instead (idle exit racing with the command) or does not answer for a very long time.
bool box_wait(ydc_context* c, int g, uint32_t seq, uint32_t* word) {
  const unsigned long long* p = &c->h_box->reply[g];
  for (uint32_t spins = 0;; ++spins) {
    const unsigned long long v = box_load(p);
    if ((uint32_t)(v >> 32) == seq) {
      *word = (uint32_t)v;
      return true;
    }
    if ((spins & 0x3FFF) == 0x3FFF) {
      if (__atomic_load_n(&c->h_box->alive, __ATOMIC_ACQUIRE) == 0) {
        // (it may have answered right before leaving)
        const unsigned long long w = box_load(p);
        if ((uint32_t)(w >> 32) == seq) {
          *word = (uint32_t)w;
          return true;
        }
        return false;
      }
      // A live kernel that is slow (a preempted GPU, a debugger) is waited for: giving it up and
      // sending the command again could apply its releases and commit its picks twice. Only a
      // stream that has ended — finished or faulted — ends the wait.
      if ((spins & 0xFFFFF) == 0xFFFFF && hipStreamQuery(c->res_stream) != hipErrorNotReady) {
        const unsigned long long w = box_load(p);
        if ((uint32_t)(w >> 32) == seq) {
          *word = (uint32_t)w;
          return true;
        }
        return false;
      }
    }
  }
}

void resident_forget(ydc_context* c) {
  c->res_live = false;
  std::lock_guard<std::mutex> lk(g_resident_mu);
  g_resident.erase(std::remove(g_resident.begin(), g_resident.end(), c), g_resident.end());
}

// Ends the context's resident kernel (if any): QUIT through the mailbox, then its stream. After
// this the registry columns in HBM are what every other path expects (the kernel writes
// running_tasks and heartbeat rows through after every command).
void resident_stop(ydc_context* c) {
  if (!c->res_live) return;
  if (__atomic_load_n(&c->h_box->alive, __ATOMIC_ACQUIRE) != 0) {
    if (++c->tick_seq == 0) c->tick_seq = 1;
    const uint32_t seq = c->tick_seq;
    for (int g = 15; g >= 0; --g)
      __atomic_store_n(&c->h_box->head[g], ((unsigned long long)seq << 32) | (g == 0 ? kTickCmdQuit : 0u),
                       __ATOMIC_RELEASE);
    uint32_t word;
    (void)box_wait(c, 0, seq, &word);
  }
  (void)hipStreamSynchronize(c->res_stream);
  resident_forget(c);
}

void resident_atexit() {
  std::vector<ydc_context*> live;
  {
    std::lock_guard<std::mutex> lk(g_resident_mu);
    live = g_resident;
  }
  for (auto* c : live) resident_stop(c);
}

int resident_prepare(ydc_context* c) {
  if (!c->h_box) {
    HIP_TRY(c, c->h_box.reserve(sizeof(TickBox)));
    std::memset(c->h_box, 0, sizeof(TickBox));
  }
  HIP_TRY(c, c->res_stream.create());
  HIP_TRY(c, c->res_ev.create(hipEventDisableTiming));
  return YDC_OK;
}

struct TickCall {
  const ydc_task_soa* tasks = nullptr;  // host columns, or device addresses (tasks_on_device)
  bool tasks_on_device = false;
  uint32_t n_tasks = 0;
  const uint32_t* upd_idx = nullptr;  // host; rows known to change no structure
  const ydc_servant_row* upd_rows = nullptr;
  uint32_t n_upd = 0;
  const uint32_t* rel = nullptr;  // host
  uint32_t n_rel = 0;
  uint32_t flags = 0;
  uint32_t* out_idx = nullptr;  // host, or device addresses (out_on_device)
  double* out_util = nullptr;
  uint32_t* out_running = nullptr;
  bool out_on_device = false;
};


// Fills the context's stats after a tick.
void tick_stats(ydc_context* c, uint32_t N, uint32_t granted, uint32_t timeouts, uint32_t env_not_found) {
  ++c->tick_batches;
  ydc_stats& st = c->stats;
  std::memset(&st, 0, sizeof(st));
  st.n_tasks = N;
  st.n_servants = c->reg.n;
  st.n_classes = c->tables.n_classes();
  st.key_bits = c->kf.key_bits;
  st.n_chunks = 1;
  st.rounds = 1;
  st.chunk_sims = 1;
  st.small_batch = 1;
  st.granted = granted;
  st.timeouts = timeouts;
  st.env_not_found = env_not_found;
}

// The answer of a resident kernel to command `seq`: counters, placements (tick_kernel.h: TickBox).
// false: the kernel left without taking the command.
bool resident_receive(ydc_context* c, const TickCall& io, uint32_t seq) {
  const uint32_t N = io.n_tasks;
  uint32_t counters;
  if (!box_wait(c, 0, seq, &counters)) return false;
  if (N <= 7 && !io.out_util) {
    for (uint32_t i = 0; i < N; ++i)
      if (!box_wait(c, 1 + (int)i, seq, &io.out_idx[i])) return false;
  } else {
    // (the arrays were stored, and fenced, ahead of the granules)
    for (uint32_t i = 0; i < N; ++i) io.out_idx[i] = __atomic_load_n(&c->h_box->out_idx[i], __ATOMIC_RELAXED);
    if (io.out_util) std::memcpy(io.out_util, c->h_box->out_util, (size_t)N * 8);
  }
  // granted: the requests that are neither of the two (the counters are bytes; N <= 64 fits)
  const uint32_t timeouts = (counters >> 8) & 0xFF, envnf = (counters >> 16) & 0xFF;
  tick_stats(c, N, N - timeouts - envnf, timeouts, envnf);
  return true;
}

int tick_run(ydc_context* c, const TickCall& io) {
  const uint32_t S = c->reg.n, C = c->tables.n_classes(), N = io.n_tasks;
  const uint32_t W = std::max<uint32_t>(1, ceil_div(C, 64));
  const bool commit0 = (io.flags & YDC_DISPATCH_COMMIT) != 0;
  // The resident form takes what a scheduler's turn looks like: COMMIT, host buffers, everything
  // within what travels as arguments.
  const bool resident = c->opt_resident && commit0 && !io.tasks_on_device && !io.out_on_device && !io.out_running &&
                        N <= kTickInlineTasks && io.n_upd <= kTickInlineUpd && io.n_rel <= kTickInlineRel &&
                        !c->profiling;
  if (c->res_live && !resident) resident_stop(c);
  // A resident kernel answers with or without utilisations for its whole life (its out_util is a
  // launch argument): a call that wants the other kind ends it and launches its own.
  if (c->res_live && (io.out_util != nullptr) != c->res_util) resident_stop(c);
  if (c->res_live) {
    TickBox* b = c->h_box;
    if (__atomic_load_n(&b->alive, __ATOMIC_ACQUIRE) != 0) {
      if (++c->tick_seq == 0) c->tick_seq = 1;
      const uint32_t seq = c->tick_seq;
      // Payload beyond the head first, the head's eight granules last. (One RPC's requests are
      // copies of one another, scheduler_service_impl.cc:228-264: then the head says so and holds all.)
      bool same = N > 1;
      for (uint32_t i = 1; i < N && same; ++i)
        same = io.tasks->env_id[i] == io.tasks->env_id[0] && io.tasks->min_version[i] == io.tasks->min_version[0] &&
               io.tasks->requestor_ip[i] == io.tasks->requestor_ip[0];
      if (N > 1 && !same)
        for (uint32_t i = 0; i < N; ++i) {
          b->env[i] = io.tasks->env_id[i];
          b->minv[i] = io.tasks->min_version[i];
          b->rip[i] = io.tasks->requestor_ip[i];
        }
      if (io.n_rel > 7) std::memcpy(b->rel, io.rel, (size_t)io.n_rel * 4);
      if (io.n_upd > 1)
        for (uint32_t i = 0; i < io.n_upd; ++i) {
          b->upd_idx[i] = io.upd_idx[i];
          b->upd[i] = TickRow{io.upd_rows[i].num_processors, io.upd_rows[i].current_load, io.upd_rows[i].max_tasks,
                              io.upd_rows[i].flags};
        }
      uint32_t words[16] = {kTickCmdTick | (same ? kTickCmdSame : 0u) | (N << 8) | (io.n_upd << 16) | (io.n_rel << 24),
                            N ? io.tasks->env_id[0] : 0u, N ? io.tasks->min_version[0] : 0u,
                            N ? io.tasks->requestor_ip[0] : 0u};
      for (uint32_t j = 0; j < 4 && j < io.n_rel; ++j) words[4 + j] = io.rel[j];
      for (uint32_t j = 4; j < 7 && j < io.n_rel; ++j) words[9 + j] = io.rel[j];
      if (io.n_upd) {
        words[8] = io.upd_idx[0];
        words[9] = io.upd_rows[0].num_processors;
        words[10] = io.upd_rows[0].current_load;
        words[11] = io.upd_rows[0].max_tasks;
        words[12] = io.upd_rows[0].flags;
      }
      for (int g = 15; g >= 0; --g)
        __atomic_store_n(&b->head[g], ((unsigned long long)seq << 32) | words[g], __ATOMIC_RELEASE);
      if (resident_receive(c, io, seq)) {
        ++c->tick_resident;
        return YDC_OK;
      }
    }
    // The kernel has left (nobody asked for a while): its stream is drained, a new one is launched
    // with this very command.
    HIP_TRY(c, hipStreamSynchronize(c->res_stream));
    resident_forget(c);
  }
  if (resident)
    if (int rc = resident_prepare(c)) return rc;
  if (!c->h_tick_done) {
    HIP_TRY(c, c->h_tick_done.reserve(sizeof(TickDone)));
    std::memset(c->h_tick_done, 0, sizeof(TickDone));
  }
  auto pad = [](size_t b) { return (b + 63) & ~(size_t)63; };
  // Arena: [request columns] [heartbeat indexes | rows] [released] | [idx] [utilisation]
  const bool tasks_ptr = !io.tasks_on_device && N > kTickInlineTasks;
  const bool upd_ptr = io.n_upd > kTickInlineUpd, rel_ptr = io.n_rel > kTickInlineRel;
  const size_t o_env = 0, o_upd = o_env + (tasks_ptr ? 3 * pad((size_t)N * 4) : 0);
  const size_t o_rows = o_upd + (upd_ptr ? pad((size_t)io.n_upd * 4) : 0);
  const size_t o_rel = o_rows + (upd_ptr ? pad((size_t)io.n_upd * sizeof(TickRow)) : 0);
  const size_t o_idx = o_rel + (rel_ptr ? pad((size_t)io.n_rel * 4) : 0);
  const size_t o_util = o_idx + (io.out_on_device ? 0 : pad((size_t)N * 4));
  const size_t need = o_util + (!io.out_on_device && io.out_util ? pad((size_t)N * 8) : 0);
  if (need > c->h_tick_io.cap) HIP_TRY(c, c->h_tick_io.reserve(std::max<size_t>(need + need / 2, 8192)));
  const bool commit = (io.flags & YDC_DISPATCH_COMMIT) != 0;
  TickArgs a;
  a.nproc = c->d_nproc.p;
  a.load = c->d_load.p;
  a.max_tasks = c->d_max_tasks.p;
  a.flags = c->d_flags.p;
  a.class_of = c->d_class_of.p;
  a.ip = c->d_ip.p;
  a.running = c->d_running.p;
  a.cls_env = c->d_cls_env.p;
  a.cls_ver = c->d_cls_ver.p;
  a.S = S;
  a.C = C;
  a.EW = c->reg.env_words;
  a.W = W;
  // running_tasks: the picks work on the resident column (COMMIT) or on a copy of it.
  uint32_t* dev_run_out = io.out_running ? (io.out_on_device ? io.out_running : c->d_running_out.p) : nullptr;
  a.rw = commit ? c->d_running.p : (dev_run_out ? dev_run_out : c->d_running_out.p);
  a.run_out = dev_run_out && dev_run_out != a.rw ? dev_run_out : nullptr;
  a.n_tasks = N;
  a.t_env = a.t_minv = a.t_rip = nullptr;
  if (io.tasks_on_device) {
    a.t_env = io.tasks->env_id;
    a.t_minv = io.tasks->min_version;
    a.t_rip = io.tasks->requestor_ip;
  } else if (tasks_ptr) {
    const size_t col = pad((size_t)N * 4);
    std::memcpy(c->h_tick_io.p + o_env, io.tasks->env_id, (size_t)N * 4);
    std::memcpy(c->h_tick_io.p + o_env + col, io.tasks->min_version, (size_t)N * 4);
    std::memcpy(c->h_tick_io.p + o_env + 2 * col, io.tasks->requestor_ip, (size_t)N * 4);
    a.t_env = (const uint32_t*)(c->h_tick_io.z + o_env);
    a.t_minv = (const uint32_t*)(c->h_tick_io.z + o_env + col);
    a.t_rip = (const uint32_t*)(c->h_tick_io.z + o_env + 2 * col);
  } else {
    for (uint32_t i = 0; i < N; ++i) {
      a.in_env[i] = io.tasks->env_id[i];
      a.in_minv[i] = io.tasks->min_version[i];
      a.in_rip[i] = io.tasks->requestor_ip[i];
    }
  }
  a.n_upd = io.n_upd;
  a.upd_idx = nullptr;
  a.upd_rows = nullptr;
  {
    uint32_t* idx = upd_ptr ? (uint32_t*)(c->h_tick_io.p + o_upd) : a.in_upd_idx;
    TickRow* rows = upd_ptr ? (TickRow*)(c->h_tick_io.p + o_rows) : a.in_upd;
    for (uint32_t i = 0; i < io.n_upd; ++i) {
      idx[i] = io.upd_idx[i];
      rows[i] = TickRow{io.upd_rows[i].num_processors, io.upd_rows[i].current_load, io.upd_rows[i].max_tasks,
                        io.upd_rows[i].flags};
    }
    if (upd_ptr) {
      a.upd_idx = (const uint32_t*)(c->h_tick_io.z + o_upd);
      a.upd_rows = (const TickRow*)(c->h_tick_io.z + o_rows);
    }
  }
  a.n_rel = io.n_rel;
  a.rel = nullptr;
  if (rel_ptr) {
    std::memcpy(c->h_tick_io.p + o_rel, io.rel, (size_t)io.n_rel * 4);
    a.rel = (const uint32_t*)(c->h_tick_io.z + o_rel);
  } else if (io.n_rel) {
    std::memcpy(a.in_rel, io.rel, (size_t)io.n_rel * 4);
  }
  a.out_idx = io.out_on_device ? io.out_idx : (uint32_t*)(c->h_tick_io.z + o_idx);
  a.out_util = io.out_util ? (io.out_on_device ? io.out_util : (double*)(c->h_tick_io.z + o_util)) : nullptr;
  a.done = c->h_tick_done.dev();
  a.box = nullptr;
  a.idle_ticks = 0;
  if (++c->tick_seq == 0) c->tick_seq = 1;
  a.seq = c->tick_seq;
  hipStream_t launch_stream = c->stream;
  if (resident) {
    // This launch stays: it answers through the mailbox like every later command, on a stream of
    // its own, behind whatever the context's stream still has in flight.
    a.box = c->h_box.dev();
    a.idle_ticks = (unsigned long long)c->opt_resident_idle_ms * 100000ull;
    a.out_idx = c->h_box.dev()->out_idx;
    a.out_util = io.out_util ? c->h_box.dev()->out_util : nullptr;
    __atomic_store_n(&c->h_box->alive, 1u, __ATOMIC_RELEASE);
    HIP_TRY(c, hipEventRecord(c->res_ev, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->res_stream, c->res_ev, 0));
    launch_stream = c->res_stream;
  }

  if (c->profiling) {
    c->ksamples_used = 0;
    for (int s = 0; s <= 6; ++s) mark(c, s);
  }
  // As few waves as hold the registry in registers (tick_kernel.h): 256 threads with up to 16
  // servants each up to 4096 servants, 512 threads above 4096 (32 per thread above 8192).
  const uint32_t per_thread = std::max(1u, ceil_div(S, 256u));
  // LDS: the eligible-class mask, the candidate lists of the merge (the builds tick_merges names,
  // 32 B per thread), the servants' hosts and classes (6 B per servant slot).
  auto launch = [&](auto kernel, uint32_t threads, uint32_t k, bool pk) -> int {
    const size_t lds = (size_t)W * 8 + (tick_merges((int)threads, (int)k, pk) ? (size_t)32 * threads : 0) +
                       (size_t)6 * threads * k;
    if (lds > 48 * 1024)
      HIP_TRY(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    YDC_LAUNCH(c, "k_tick", kernel, dim3(1), dim3(threads), lds, launch_stream, a);
    return YDC_OK;
  };
  uint32_t idx_bits = 1;
  const bool packed = tick_packed(c, &idx_bits);
  a.cap_bits = c->tables.cap_bits;
  a.idx_bits = idx_bits;
  int lrc;
#define YDC_TICK_LAUNCH(T, KK, COLD) \
  lrc = packed ? launch(k_tick<T, KK, COLD, true>, T, KK, true) : launch(k_tick<T, KK, COLD, false>, T, KK, false)
  if (per_thread <= 1) YDC_TICK_LAUNCH(256, 1, true);
  else if (per_thread <= 2) YDC_TICK_LAUNCH(256, 2, true);
  else if (per_thread <= 4) YDC_TICK_LAUNCH(256, 4, true);
  else if (per_thread <= 8) YDC_TICK_LAUNCH(256, 8, true);
  else if (per_thread <= 16) YDC_TICK_LAUNCH(256, 16, true);
  else if (per_thread <= 32) YDC_TICK_LAUNCH(512, 16, true);
  else YDC_TICK_LAUNCH(512, 32, false);
#undef YDC_TICK_LAUNCH
  if (lrc) return lrc;
  HIP_TRY(c, hipGetLastError());
  mark(c, 7);
  ++c->tick_launches;
  if (resident) {
    c->res_live = true;
    c->res_util = io.out_util != nullptr;
    {
      std::lock_guard<std::mutex> lk(g_resident_mu);
      g_resident.push_back(c);
      if (!g_resident_atexit) {
        g_resident_atexit = true;
        std::atexit(resident_atexit);
      }
    }
    if (!resident_receive(c, io, a.seq)) {
      (void)hipStreamSynchronize(c->res_stream);
      resident_forget(c);
      return fail(c, YDC_ERR_HIP, "the resident small-batch kernel left without answering its first command");
    }
    return YDC_OK;
  }

  // The kernel's last store is the stamp; spin on it (a launch-to-stamp round trip is a third
  // shorter than launch + hipStreamSynchronize). Never forever: the stream is asked now and then.
  {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; ++spins) {
      if (__atomic_load_n(&c->h_tick_done->seq, __ATOMIC_ACQUIRE) == a.seq) break;
      if ((spins & 0xFFFF) == 0xFFFF) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q != hipSuccess && q != hipErrorNotReady)
          return fail(c, YDC_ERR_HIP, "the small-batch kernel failed: %s", hipGetErrorString(q));
        if (q == hipSuccess && __atomic_load_n(&c->h_tick_done->seq, __ATOMIC_ACQUIRE) != a.seq)
          return fail(c, YDC_ERR_HIP, "the small-batch kernel finished without its stamp");
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
          return fail(c, YDC_ERR_HIP, "no stamp from the small-batch kernel after 30 s");
      }
    }
  }
  if (io.out_on_device || (io.out_running && !io.out_on_device) || c->profiling)
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (device outputs: complete when the call returns)
  if (!io.out_on_device) {
    if (N) std::memcpy(io.out_idx, c->h_tick_io.p + o_idx, (size_t)N * 4);
    if (N && io.out_util) std::memcpy(io.out_util, c->h_tick_io.p + o_util, (size_t)N * 8);
    if (io.out_running && S)
      HIP_TRY(c, hipMemcpy(io.out_running, dev_run_out, (size_t)S * 4, hipMemcpyDeviceToHost));
  }
  tick_stats(c, N, c->h_tick_done->granted, c->h_tick_done->timeouts, c->h_tick_done->env_not_found);
  ydc_stats& st = c->stats;
  if (c->profiling) {
    for (int i = 0; i < 7; ++i) (void)hipEventElapsedTime(&st.stage_ms[i], c->ev[i], c->ev[i + 1]);
    (void)hipEventElapsedTime(&st.stage_ms[YDC_STAGE_TOTAL], c->ev[0], c->ev[7]);
    collect_kernel_profile(c);
  }
  return YDC_OK;
}

// One batch whose request columns (tk) and outputs are device addresses, placed when this returns:
// the body of ydc_dispatch_device, and what ydc_dispatch hands its staged call to.
int dispatch_batch(ydc_context* c, const ydc_task_soa* tk, uint32_t N, const BatchCall& call) {
  if (c->max_tasks && N > c->max_tasks)
    return fail(c, YDC_ERR_CAPACITY, "%u tasks > max_tasks %u", N, c->max_tasks);
  if (c->pend_count && !c->pend[c->pend_head].rerun && c->pend[c->pend_head].active && !call.replay)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "pipelined batches outstanding: ydc_dispatch_wait first");
  HIP_TRY(c, hipSetDevice(c->device));
  if (N && N <= c->small_batch() && call.out_idx && !call.staged()) {
    // A handful of requests: one launch of the one-workgroup kernel (tick_kernel.h).
    if (c->tables_dirty)
      if (int rc = rebuild_tables(c)) return rc;
    if (tick_takes(c, N)) {
      TickCall io;
      io.tasks = tk;
      io.tasks_on_device = true;
      io.n_tasks = N;
      io.flags = call.flags;
      io.out_idx = call.out_idx;
      io.out_util = call.out_util;
      io.out_running = call.out_running;
      io.out_on_device = true;
      return tick_run(c, io);
    }
  }
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  BatchPlan p;
  uint32_t rounds = 0;
  if (int rc = place_batch(c, N, tk, call, &p, &rounds)) return rc;
  fill_stats(c, p, rounds);
  ydc_stats& s = c->stats;
  if (c->profiling) {
    for (int i = 0; i < 7; ++i) (void)hipEventElapsedTime(&s.stage_ms[i], c->ev[i], c->ev[i + 1]);
    (void)hipEventElapsedTime(&s.stage_ms[YDC_STAGE_TOTAL], c->ev[0], c->ev[7]);
    collect_kernel_profile(c);
  }
  return YDC_OK;
}

}  // namespace

extern "C" {

int ydc_dispatch_device(ydc_context* c, const ydc_task_soa* tk, uint32_t N, uint32_t flags,
                        uint32_t* d_out_idx, double* d_out_util, uint32_t* d_out_running) {
  if (!c || (N && !tk)) return YDC_ERR_INVALID_ARGUMENT;
  join_lanes(c);
  return dispatch_batch(c, tk, N, batch_call(c, flags, d_out_idx, d_out_util, d_out_running, c->h_prm.dev()));
}

namespace {
// A pipelined batch whose event has completed: it took no effect (not final within its launches,
// a bin sort's window missed, the latch of its lane was set, or its slots overflowed).
bool outcome_missed(const ydc_context::Pending& pd) {
  const DeviceParams& o = *pd.h_outcome.get();
  return o.overflow || o.pipeline_broken || (pd.plan.binsort && o.window_miss) ||
         o.n_changed[(pd.launched - 1) & 63] != 0;
}
}  // namespace

// Pipelined form of ydc_dispatch_device: enqueues the whole batch (front, the matching passes the
// last batches needed, the gated finalise, the outcome read-back) and returns; the host looks at
// the outcome in ydc_dispatch_wait — by then the next batch is already queued behind this one, so
// the device does not idle while the host turns around. Exact whatever happens: a batch that is
// not final within its pre-launched passes (or whose bins overflowed) takes no effect, latches
// DeviceParams::pipeline_broken so that the batch behind it takes none either, and both are
// replayed in order by ydc_dispatch_wait. A batch that does not depend on the outstanding one is
// enqueued on the other lane and runs beside it (lane_rule.h).
int ydc_dispatch_device_async(ydc_context* c, const ydc_task_soa* tk, uint32_t N, uint32_t flags,
                              uint32_t* d_out_idx, double* d_out_util, uint32_t* d_out_running) {
  if (!c || (N && !tk)) return YDC_ERR_INVALID_ARGUMENT;
  if (c->pend_count == 2) return fail(c, YDC_ERR_INVALID_ARGUMENT, "two batches outstanding: ydc_dispatch_wait first");
  if (c->max_tasks && N > c->max_tasks)
    return fail(c, YDC_ERR_CAPACITY, "%u tasks > max_tasks %u", N, c->max_tasks);
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  auto& pd = c->pend[(c->pend_head + c->pend_count) & 1];
  HIP_TRY(c, pd.h_outcome.reserve(sizeof(DeviceParams)));
  HIP_TRY(c, pd.ev.create(hipEventDisableTiming));
  pd.active = true;
  pd.rerun = false;
  pd.tk = tk ? *tk : ydc_task_soa{};
  pd.n = N;
  pd.flags = flags;
  pd.out_idx = d_out_idx;
  pd.out_util = d_out_util;
  pd.out_running = d_out_running;
  pd.launched = 0;
  // Which lane (lane_rule.h). Whether the plan will take the enqueued path below is known from
  // the tables: plan_batch must already run under the lane's scope, its views are the lane's.
  ydc_context::Pending* const ahead = c->pend_count == 1 ? &c->pend[c->pend_head] : nullptr;
  const uint32_t n_cls = c->tables_dirty ? 0u : c->tables.n_classes();
  pd.lb = LaneBatch{};
  pd.lb_epoch = c->lane0_epoch;
  pd.lb.commit = (flags & YDC_DISPATCH_COMMIT) != 0;
  pd.lb.enqueued = !(ahead && ahead->rerun) && N && n_cls && n_cls <= kMaxWaveClasses && !c->profiling &&
                   !c->debug_verify_binsort;
  pd.lb.out[0] = LaneOutput{d_out_idx, (size_t)N * 4};
  pd.lb.out[1] = LaneOutput{d_out_util, (size_t)N * 8};
  pd.lb.out[2] = LaneOutput{d_out_running, (size_t)c->reg.n * 4};
  LaneChoice lane;
  if (ahead) {
    ahead->lb.enqueued = !ahead->rerun;
    const LaneContext lc{c->opt_lanes, c->own_stream.s != nullptr, c->group.n_ranks != 0 || c->group.via != nullptr,
                         c->stream_mode.active, c->lane0_settled()};
    lane = lane_for(lc, &ahead->lb, pd.lb);
  }
  if (lane.wait_first) {
    // Behind a batch on lane 1 without an event between the lanes: the host waits for it. If it
    // took no effect, neither may this one (on lane 0 it does not see lane 1's latch): both are
    // replayed in order by ydc_dispatch_wait.
    if (hipEventSynchronize(ahead->ev) != hipSuccess) {
      pd.active = false;
      return fail(c, YDC_ERR_HIP, "could not wait for the batch on the second lane");
    }
    if (outcome_missed(*ahead)) ahead->rerun = true;
  }
  if (lane.lane == 1)
    if (int rc = lane1_prepare(c)) {
      pd.active = false;
      return rc;
    }
  pd.lb.lane = lane.lane;
  const LaneScope scope(c, lane.lane);
  // A batch behind one that already has to be replayed is not worth enqueueing.
  const bool behind_rerun = ahead && ahead->rerun;
  // A batch that cannot be enqueued completely is not outstanding: nothing of it can take effect
  // without its finalise, which is enqueued last; the slot is free again.
  auto give_up = [&](int rc) {
    pd.active = false;
    return rc;
  };
  // (beside: a context that may use the second lane at all — this batch or the next one behind it)
  const bool beside = c->opt_lanes && c->own_stream.s != nullptr && c->group.n_ranks == 0 && c->group.via == nullptr &&
                      !c->stream_mode.active;
  if (int rc = plan_batch(c, N, &pd.plan, false, beside)) return give_up(rc);
  if (behind_rerun || !pd.plan.wave_path || c->profiling || c->debug_verify_binsort) {
    // (registries without the wave path have host-checked rounds: placed when waited for)
    pd.rerun = true;
    pd.lb.lane = 0;
  } else {
    // (the outcome block: stored by k_finalize's last servant workgroup; a registry without
    // servants has none, then it is read back with a copy)
    BatchCall call = batch_call(c, flags, d_out_idx, d_out_util, d_out_running, pd.h_outcome.dev());
    call.pipelined = true;
    const bool outcome_stored = call.outcome != nullptr;
    if (int rc = enqueue_front(c, pd.plan, &pd.tk, call)) return give_up(rc);
    const uint32_t group = first_group(c, pd.plan);
    for (uint32_t r = 0; r < group; ++r) enqueue_pass(c, pd.plan, r, 1u);
    pd.launched = group;
    if (int rc = enqueue_finalize(c, pd.plan, call, (group - 1) & 63)) return give_up(rc);
    // (a batch that turns out not to be final wrote the column's own values: the exchange is
    // harmless then, and the replay plans with the pointers as they are)
    if (call.by_swap) std::swap(c->d_running, c->d_running_out);
    // (from here on the batch may take effect: a failing copy / event leaves it to be waited for
    // the slow way — a stream synchronise instead of the event)
    if ((!outcome_stored &&
         hipMemcpyAsync(pd.h_outcome, c->d_prm.p, sizeof(DeviceParams), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipEventRecord(pd.ev, c->stream) != hipSuccess) {
      (void)hipStreamSynchronize(c->stream);
      return give_up(fail(c, YDC_ERR_HIP, "could not enqueue the outcome read-back of a pipelined batch"));
    }
    if (lane.lane == 1) ++c->lane1_batches;
  }
  ++c->pend_count;
  return YDC_OK;
}

// Waits for the OLDEST outstanding batch; its results are final when this returns.
int ydc_dispatch_wait(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (c->pend_count == 0) return fail(c, YDC_ERR_INVALID_ARGUMENT, "no batch outstanding");
  HIP_TRY(c, hipSetDevice(c->device));
  auto& pd = c->pend[c->pend_head];
  auto pop = [&] {
    pd.active = false;
    c->pend_head ^= 1;
    --c->pend_count;
  };
  // Both lanes idle and the latch of this batch's lane cleared; the batch behind it on the same
  // lane took no effect either and is replayed when it is waited for. One on the other lane was
  // enqueued as independent of this one: it has taken effect validly and stays as it is.
  auto drain = [&]() -> int {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->lane1) HIP_TRY(c, hipStreamSynchronize(c->lane1->stream));
    const bool second = pd.lb.lane == 1 && c->lane1;
    HIP_TRY(c, hipMemsetAsync(&(second ? c->lane1->d_prm : c->d_prm).p->pipeline_broken, 0, 4,
                              second ? c->lane1->stream : c->stream));
    auto& behind = c->pend[c->pend_head ^ 1];
    if (c->pend_count == 2 && behind.lb.lane == pd.lb.lane) behind.rerun = true;
    return YDC_OK;
  };
  bool miss = pd.rerun;
  uint32_t rounds = 0;
  if (!miss) {
    HIP_TRY(c, hipEventSynchronize(pd.ev));
    const DeviceParams& o = *pd.h_outcome.get();
    if (o.overflow) {
      // Took no effect and latched the pipeline (k_finalize's gate includes overflow for
      // pipelined batches), so the batch behind it has not taken any either: drain, clear the
      // latch, leave that batch to be replayed when it is waited for, report this one.
      const uint32_t bound = pd.plan.slot_bound;
      if (int rc = drain()) return rc;
      pop();
      return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", bound);
    }
    miss = o.pipeline_broken || (pd.plan.binsort && o.window_miss) || o.n_changed[(pd.launched - 1) & 63] != 0;
    if (!miss) {
      rounds = pd.launched;
      for (uint32_t r = 0; r < pd.launched; ++r)
        if (o.n_changed[r & 63] == 0) {
          rounds = r + 1;
          break;
        }
      *c->h_prm = o;
      c->round_hint = rounds;
      zone_feedback(c, pd.plan, o, rounds);
      fill_stats(c, pd.plan, rounds);
      if (pd.lb.lane == 0) c->lane0_seen = pd.lb_epoch;
      pop();
      return YDC_OK;
    }
  }
  // Not final in the pipeline (or never enqueued): nothing of this batch — nor of the one behind
  // it on its lane — has taken effect. Drain, clear the latch, place it the synchronous way; the
  // batch behind it is replayed when it is waited for.
  ++c->pipeline_misses;
  if (int rc = drain()) return rc;
  const ydc_task_soa tk = pd.tk;
  const uint32_t n = pd.n, flags = pd.flags;
  uint32_t* oi = pd.out_idx;
  double* ou = pd.out_util;
  uint32_t* orun = pd.out_running;
  pop();
  BatchCall call = batch_call(c, flags, oi, ou, orun, c->h_prm.dev());
  call.replay = true;
  const int rc = dispatch_batch(c, &tk, n, call);
  if (rc == YDC_OK) c->lane0_seen = c->lane0_epoch;  // (placed and complete, on lane 0)
  return rc;
}

int ydc_dispatch(ydc_context* c, const ydc_task_soa* tk, uint32_t N, uint32_t flags,
                 uint32_t* out_idx, double* out_util, uint32_t* out_running) {
  if (!c || (N && (!tk || !out_idx))) return YDC_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  const bool same = N <= kTickBlock && tick_same_requests(tk, N);
  if (N && N <= c->small_batch(same)) {
    // A handful of requests: one launch of the one-workgroup kernel, the requests as kernel
    // arguments, the results stored to page-locked memory (tick_kernel.h).
    if (c->max_tasks && N > c->max_tasks)
      return fail(c, YDC_ERR_CAPACITY, "%u tasks > max_tasks %u", N, c->max_tasks);
    if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "pipelined batches outstanding: ydc_dispatch_wait first");
    if (c->tables_dirty)
      if (int rc = rebuild_tables(c)) return rc;
    if (tick_takes(c, N, same)) {
      TickCall io;
      io.tasks = tk;
      io.n_tasks = N;
      io.flags = flags;
      io.out_idx = out_idx;
      io.out_util = out_util;
      io.out_running = out_running;
      return tick_run(c, io);
    }
  }
  const uint32_t S = c->reg.n;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // Page-locked caller buffers (ydc_host_register / ydc_host_alloc) are used as they are: the
  // classification reads the request columns and k_finalize writes the results through their
  // device addresses — no staging memcpy, no copy command on either side.
  const uint32_t* m_in[3] = {nullptr, nullptr, nullptr};
  if (N) {
    m_in[0] = (const uint32_t*)pinned_device_pointer(tk->env_id, (size_t)N * 4);
    m_in[1] = m_in[0] ? (const uint32_t*)pinned_device_pointer(tk->min_version, (size_t)N * 4) : nullptr;
    m_in[2] = m_in[1] ? (const uint32_t*)pinned_device_pointer(tk->requestor_ip, (size_t)N * 4) : nullptr;
  }
  const bool in_pinned = m_in[0] && m_in[1] && m_in[2];
  uint32_t* m_idx = N ? (uint32_t*)pinned_device_pointer(out_idx, (size_t)N * 4) : nullptr;
  uint32_t* m_run = out_running && S ? (uint32_t*)pinned_device_pointer(out_running, (size_t)S * 4) : nullptr;
  double* m_util = out_util && N ? (double*)pinned_device_pointer(out_util, (size_t)N * 8) : nullptr;
  const bool out_pinned = (!N || m_idx) && (!(out_running && S) || m_run) && (!(out_util && N) || m_util);
  // in: env | min_version | requestor_ip        out: idx | running_tasks | utilisation
  const size_t col = pad((size_t)N * 4), in_bytes = 3 * col;
  const size_t o_run = pad((size_t)N * 4), o_util = o_run + pad((size_t)(out_running ? S : 0) * 4);
  const size_t res_bytes = o_util + (out_util ? (size_t)N * 8 : 0);
  // (the staging arenas grow by half as much again as is asked for)
  auto arena = [](PinnedBuf& b, size_t want) {
    return want <= b.cap ? hipSuccess : b.reserve(std::max<size_t>(want + want / 2, 4096), hipHostMallocDefault);
  };
  // Request columns: read in place (in_pinned), or staged through the context's own pinned arena
  // (pageable caller memory).
  ydc_task_soa d{};
  BatchCall call = batch_call(c, flags, m_idx, out_util ? m_util : nullptr, out_running && S ? m_run : nullptr,
                              c->h_prm.dev());
  if (in_pinned) {
    d = ydc_task_soa{m_in[0], m_in[1], m_in[2]};
  } else if (N) {
    HIP_TRY(c, arena(c->h_in, in_bytes));
    HIP_TRY(c, c->d_in.reserve(std::max<size_t>(in_bytes, 256)));
    HIP_TRY(c, c->copy_stream.create());
    HIP_TRY(c, c->copy_ev.create(hipEventDisableTiming));
    // The columns are staged and copied inside the batch, behind the launches that do not need
    // them (enqueue_front / stage_host_requests).
    call.host_in.tk = tk;
    call.host_in.n = N;
    call.host_in.col = col;
    call.host_in.bytes = in_bytes;
    d = ydc_task_soa{(const uint32_t*)c->d_in.p, (const uint32_t*)(c->d_in.p + col),
                     (const uint32_t*)(c->d_in.p + 2 * col)};
  }
  // (dispatch_batch waits for the stream: the results are in the caller's buffers)
  if (out_pinned) return dispatch_batch(c, &d, N, call);
  HIP_TRY(c, arena(c->h_res, res_bytes));
  HIP_TRY(c, c->d_res.reserve(std::max<size_t>(res_bytes, 256)));
  call.out_idx = (uint32_t*)c->d_res.p;
  call.out_util = out_util ? (double*)(c->d_res.p + o_util) : nullptr;
  call.out_running = out_running && S ? (uint32_t*)(c->d_res.p + o_run) : nullptr;
  call.post_copy.dst = c->h_res.p;
  call.post_copy.src = c->d_res.p;
  call.post_copy.bytes = res_bytes;
  if (int rc = dispatch_batch(c, &d, N, call)) return rc;
  // ... or in the pinned arena.
  if (N) std::memcpy(out_idx, c->h_res.p, (size_t)N * 4);
  if (out_running && S) std::memcpy(out_running, c->h_res.p + o_run, (size_t)S * 4);
  if (out_util && N) std::memcpy(out_util, c->h_res.p + o_util, (size_t)N * 8);
  return YDC_OK;
}

int ydc_dispatch_tick(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                      const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                      const uint32_t* release_servant_idx, uint32_t n_rel, const ydc_task_soa* tasks,
                      uint32_t n_tasks, uint32_t flags, uint32_t* out_servant_idx, double* out_utilization) {
  if (!c || (n_upd && (!upd_idx || !upd_rows)) || (n_rel && !release_servant_idx) ||
      (n_tasks && (!tasks || !out_servant_idx)))
    return YDC_ERR_INVALID_ARGUMENT;
  join_lanes(c);
  if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "pipelined batches outstanding: ydc_dispatch_wait first");
  if (c->max_tasks && n_tasks > c->max_tasks)
    return fail(c, YDC_ERR_CAPACITY, "%u tasks > max_tasks %u", n_tasks, c->max_tasks);
  HIP_TRY(c, hipSetDevice(c->device));
  // Heartbeats that change structure (a new servant, other environments / version / host /
  // capacity bound) take the general path, derived tables and all; so does a tick the kernel
  // does not take (a large batch, a registry beyond its limits). So do mask words beyond the
  // table's width and rows without masks on a table of several words (ydc_update_servants_wide
  // refuses those: let it say so).
  const bool wider = upd_env_masks ? env_words > c->reg.env_words : c->reg.env_words > 1;
  bool structural = false;
  for (uint32_t i = 0; i < n_upd && !structural; ++i)
    structural = wider || c->reg.structural(upd_idx[i], upd_rows[i], upd_env_masks, env_words, i);
  if (!structural && c->tables_dirty)
    if (int rc = rebuild_tables(c)) return rc;
  // (registry deltas ride in the launch only with COMMIT: running_tasks goes back once, into the
  // column the picks work on)
  const bool same = tick_same_requests(tasks, n_tasks);
  const bool fast = !structural && tick_takes(c, n_tasks, same) &&
                    ((flags & YDC_DISPATCH_COMMIT) || (!n_upd && !n_rel));
  if (!fast) {
    if (n_upd)
      if (int rc = ydc_update_servants_wide(c, upd_idx, upd_rows, upd_env_masks, env_words, n_upd)) return rc;
    n_upd = 0;
    if (c->tables_dirty)
      if (int rc = rebuild_tables(c)) return rc;
    if (!tick_takes(c, n_tasks, same) || (n_rel && !(flags & YDC_DISPATCH_COMMIT))) {
      if (n_rel)
        if (int rc = ydc_release_slots(c, release_servant_idx, n_rel)) return rc;
      if (!n_tasks) return YDC_OK;
      return ydc_dispatch(c, tasks, n_tasks, flags, out_servant_idx, out_utilization, nullptr);
    }
  }
  // (the host mirror of the columns such rows replace)
  for (uint32_t i = 0; i < n_upd; ++i) c->reg.store_light(upd_idx[i], upd_rows[i]);
  TickCall io;
  io.tasks = tasks;
  io.n_tasks = n_tasks;
  io.upd_idx = upd_idx;
  io.upd_rows = upd_rows;
  io.n_upd = n_upd;
  io.rel = release_servant_idx;
  io.n_rel = n_rel;
  io.flags = flags;
  io.out_idx = out_servant_idx;
  io.out_util = out_utilization;
  return tick_run(c, io);
}

int ydc_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return YDC_ERR_INVALID_ARGUMENT;
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_create_error(std::string("hipHostRegister: ") + hipGetErrorString(e));
    return YDC_ERR_HIP;
  }
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess || !dev) {
    (void)hipGetLastError();
    (void)hipHostUnregister(p);
    set_create_error("hipHostGetDevicePointer failed for a registered range");
    return YDC_ERR_HIP;
  }
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  g_pinned.push_back(PinnedRange{(const char*)p, bytes, (char*)dev, 0});
  g_not_pinned.clear();
  return YDC_OK;
}

int ydc_host_unregister(void* p) {
  if (!p) return YDC_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  for (size_t i = 0; i < g_pinned.size(); ++i)
    if (g_pinned[i].host == (const char*)p && g_pinned[i].kind == 0) {
      g_pinned.erase(g_pinned.begin() + (long)i);
      return hipHostUnregister(p) == hipSuccess ? YDC_OK : YDC_ERR_HIP;
    }
  return YDC_ERR_INVALID_ARGUMENT;
}

int ydc_host_alloc(size_t bytes, void** out) {
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_create_error(std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? YDC_ERR_NO_DEVICE : YDC_ERR_HIP;
  }
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess || !dev) {
    (void)hipGetLastError();
    (void)hipHostFree(p);
    return YDC_ERR_HIP;
  }
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned.push_back(PinnedRange{(const char*)p, bytes ? bytes : 1, (char*)dev, 1});
    g_not_pinned.clear();
  }
  *out = p;
  return YDC_OK;
}

int ydc_host_free(void* p) {
  if (!p) return YDC_OK;
  std::lock_guard<std::mutex> lk(g_pinned_mu);
  for (size_t i = 0; i < g_pinned.size(); ++i)
    if (g_pinned[i].host == (const char*)p && g_pinned[i].kind == 1) {
      g_pinned.erase(g_pinned.begin() + (long)i);
      return hipHostFree(p) == hipSuccess ? YDC_OK : YDC_ERR_HIP;
    }
  return YDC_ERR_INVALID_ARGUMENT;
}

}  // extern "C" (reopened below)

// ---------------------------------------------------------------------------
// Multi-GPU: rank-range sharding of one batch. The global batch is the
// concatenation, in rank order, of the slices the ranks pass to ydc_dispatch_sharded;
// every rank holds the same servant table and computes the same sorted slot lists, and
// replays only its own slice. Exchanges (all-gathers, a few hundred bytes to S*4 bytes per
// rank): the slices' consuming-request counts (level guesses), after every matching pass
// the end state of each rank's last chunk + its count of inconsistent chunks, and finally
// the per-servant slot deltas. Transport: RCCL (librccl.so.1, resolved with dlopen so
// that a single-GPU scheduler has no RCCL dependency), or — for several contexts of one
// process on one device, which is how the protocol is tested on a single-GPU box — a
// barrier + device copies; or, between processes, mailboxes in HIP IPC device memory or a
// shared host segment.
// On the host a group holds one Transport, chosen by the ydc_group_init* call that made it, and
// one Workspace; ydc_dispatch_sharded carries a ShardCall through named stages — front, pass
// group, tail, outcome — under a short loop that holds the retry policy; what the ranks have to
// compute alike is in shard_plan.h. Every rank must take the same branches and issue the same
// exchanges in the same order: a rank that did not would leave its peers waiting in-stream.
// ---------------------------------------------------------------------------
int ydc_context::Transport::settled(ydc_context* c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return YDC_OK;
}

namespace {

// A group of one exchanges with nobody: the gather is a copy (the communicator / mailbox exists,
// is reported and is released like any other; there is nothing to wait for).
int solo_gather(ydc_context* c, const void* send, void* recv, size_t bytes) {
  if (bytes) HIP_TRY(c, hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, c->stream));
  return YDC_OK;
}

// The mailbox reports a late peer only through DeviceParams::exchange_timeout (the words it
// waited for read as 0).
int late_peer(ydc_context* c) {
  return fail(c, YDC_ERR_HIP, "a peer's data did not arrive within the mailbox time-out (rank %d of %d)",
              c->group.rank, c->group.n_ranks);
}

// librccl must sit on the SAME HIP runtime as this library: a process may hold two
// (e.g. /opt/rocm's and the one bundled with a PyTorch wheel), and RCCL calls on device
// memory of the other runtime fail. So look next to the libamdhip64 this library is bound
// to first, and only then fall back to the soname.
void* open_rccl(std::string* err) {
  std::vector<std::string> names;
  Dl_info info;
  if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash);
      names.push_back(dir + "/librccl.so.1");
      names.push_back(dir + "/librccl.so");
    }
  }
  names.push_back("librccl.so.1");
  names.push_back("librccl.so");
  std::string tried;
  for (auto& n : names) {
    if (void* h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL)) return h;
    tried += n + " ";
  }
  if (err) *err = "dlopen failed for: " + tried + "(" + (dlerror() ? dlerror() : "?") + ")";
  return nullptr;
}

// librccl as this library uses it: the handle and the entry points, resolved here and nowhere
// else. An entry point the library lacks is NULL; who needs it says so.
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclCommCount) comm_count = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  bool open(std::string* err) {
    lib = open_rccl(err);
    if (!lib) return false;
    get_unique_id = (decltype(get_unique_id))dlsym(lib, "ncclGetUniqueId");
    comm_init_rank = (decltype(comm_init_rank))dlsym(lib, "ncclCommInitRank");
    all_gather = (decltype(all_gather))dlsym(lib, "ncclAllGather");
    comm_destroy = (decltype(comm_destroy))dlsym(lib, "ncclCommDestroy");
    comm_count = (decltype(comm_count))dlsym(lib, "ncclCommCount");
    error_string = (decltype(error_string))dlsym(lib, "ncclGetErrorString");
    return true;
  }
  const char* text(ncclResult_t r) const { return error_string ? error_string(r) : "?"; }
};

// RCCL: owns the dlopen handle and the communicator.
struct RcclTransport final : ydc_context::Transport {
  RcclApi api;
  ncclComm_t comm = nullptr;
  bool solo = false;  // a communicator of one rank
  ~RcclTransport() override {
    if (comm) (void)api.comm_destroy(comm);
    if (api.lib) (void)dlclose(api.lib);
  }
  int kind() const override { return YDC_TRANSPORT_RCCL; }
  int gather(ydc_context* c, const void* send, void* recv, size_t bytes) override {
    if (solo) return solo_gather(c, send, recv, bytes);
    ncclResult_t r = api.all_gather(send, recv, bytes, ncclUint8, comm, c->stream);
    if (r != ncclSuccess) return fail(c, YDC_ERR_HIP, "ncclAllGather: %s", api.text(r));
    return YDC_OK;
  }
  // Ask the communicator itself (ncclCommCount), not our own bookkeeping.
  int count(ydc_context* c, int* out) override {
    if (!api.comm_count) return YDC_OK;
    int n = 0;
    if (api.comm_count(comm, &n) != ncclSuccess) return fail(c, YDC_ERR_HIP, "ncclCommCount failed");
    *out = n;
    return YDC_OK;
  }
};

// Several contexts of one process on one device — how the protocol is tested on a single-GPU
// box: a barrier + device copies. Every rank holds a reference on the hub; the last one out
// deletes it.
struct LocalHub {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t generation = 0;
  std::vector<const void*> send;
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t gen = generation;
    if (++arrived == n) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != gen; });
    }
  }
};
struct LocalHubTransport final : ydc_context::Transport {
  std::shared_ptr<LocalHub> hub;
  int rank = 0;
  int kind() const override { return YDC_TRANSPORT_LOCAL; }
  int gather(ydc_context* c, const void* send, void* recv, size_t bytes) override {
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the send buffer is complete
    hub->send[rank] = send;
    hub->barrier();
    for (int r = 0; r < hub->n; ++r)
      HIP_TRY(c, hipMemcpyAsync((char*)recv + (size_t)r * bytes, hub->send[r], bytes, hipMemcpyDeviceToDevice,
                                c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hub->barrier();  // nobody rewrites its send buffer before everybody has read it
    return YDC_OK;
  }
};

// What a rank hands its peers (ydc_group_ipc_export; YDC_IPC_HANDLE_BYTES).
struct MailboxBlob {
  uint32_t magic, abi;
  int32_t rank, n_ranks;
  uint32_t slot_words, have_device, have_host, device_fine;
  int32_t device, pid;
  uint64_t bytes, raw_dev, raw_host;  // raw_*: the owner's own pointers (peers inside the owner's process)
  hipIpcMemHandle_t handle;
  char shm_name[64];
};
static_assert(sizeof(MailboxBlob) <= YDC_IPC_HANDLE_BYTES, "blob must fit the published size");
constexpr uint32_t kMailboxMagic = 0x79646362u;  // "ydcb"

// Own the pieces of a mailbox the way DevBuf owns an allocation. This rank's device block:
// fine-grained device memory where the runtime exports it (peer writes have to be visible to a
// kernel that is running — across devices that takes fine-grained memory), plain device memory
// otherwise (enough between processes that share one device). Zeroed. Without a handle the block
// serves peers inside this process only.
struct MailboxDevBlock {
  void* p = nullptr;
  bool fine = false, have_handle = false;
  hipIpcMemHandle_t handle{};
  MailboxDevBlock() = default;
  MailboxDevBlock(const MailboxDevBlock&) = delete;
  MailboxDevBlock& operator=(const MailboxDevBlock&) = delete;
  ~MailboxDevBlock() {
    if (p) (void)hipFree(p);
  }
  // p stays NULL where the device gives neither kind; an error only from zeroing what it gave.
  hipError_t create(size_t bytes, bool coarse_only) {
    if (!coarse_only) {
      if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) == hipSuccess) {
        if (hipIpcGetMemHandle(&handle, p) == hipSuccess) {
          have_handle = fine = true;
        } else {
          (void)hipFree(p);
          p = nullptr;
        }
      }
      (void)hipGetLastError();
    }
    if (!p) {
      if (hipMalloc(&p, bytes) == hipSuccess) have_handle = hipIpcGetMemHandle(&handle, p) == hipSuccess;
      else p = nullptr;
      (void)hipGetLastError();
    }
    return p ? hipMemset(p, 0, bytes) : hipSuccess;
  }
};
// This rank's host segment: a POSIX shared-memory segment, page-locked and mapped into the
// device's address space by every process that opens it. Zeroed; unlinked with its owner.
struct MailboxHostSegment {
  void* p = nullptr;
  size_t bytes = 0;
  char name[64] = {};
  MailboxHostSegment() = default;
  MailboxHostSegment(const MailboxHostSegment&) = delete;
  MailboxHostSegment& operator=(const MailboxHostSegment&) = delete;
  ~MailboxHostSegment() {
    if (!p) return;
    (void)hipHostUnregister(p);
    (void)munmap(p, bytes);
    (void)shm_unlink(name);
  }
  // Named after the process and the context. p stays NULL where the segment cannot be had.
  void create(const void* owner, size_t n) {
    snprintf(name, sizeof(name), "/ydc_box_%d_%llx", (int)getpid(), (unsigned long long)(uintptr_t)owner & 0xFFFFFFFFFFull);
    (void)shm_unlink(name);
    int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) return;
    void* m = MAP_FAILED;
    if (ftruncate(fd, (off_t)n) == 0) m = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    (void)close(fd);
    if (m != MAP_FAILED) {
      std::memset(m, 0, n);
      if (hipHostRegister(m, n, hipHostRegisterMapped | hipHostRegisterPortable) == hipSuccess) {
        p = m;
        bytes = n;
      } else {
        (void)hipGetLastError();
        (void)munmap(m, n);
      }
    }
    if (!p) (void)shm_unlink(name);
  }
};
// A peer's mailbox as opened in this process: its device block through the HIP IPC handle, or its
// host segment mapped and page-locked here. (Neither for this rank itself and for a peer inside
// this process, which are reached through their owner's pointers.)
struct MailboxPeerMap {
  void* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  MailboxPeerMap() = default;
  MailboxPeerMap(const MailboxPeerMap&) = delete;
  MailboxPeerMap& operator=(const MailboxPeerMap&) = delete;
  ~MailboxPeerMap() { close(); }
  void close() {
    if (dev) (void)hipIpcCloseMemHandle(dev);
    dev = nullptr;
    if (host) {
      (void)hipHostUnregister(host);
      (void)munmap(host, bytes);
    }
    host = nullptr;
  }
};

// Inter-process mailbox (kernels.h: k_mailbox_all_gather): this rank's mailbox in both flavours
// and the peers' as mapped into this process. Two phases: ydc_group_ipc_export makes it with the
// rank's own blocks (flavour 0, the context is not in a group yet); ydc_group_init_ipc maps the
// peers' in one flavour — and once more in the other where a rank could not open a peer's handle.
struct MailboxTransport final : ydc_context::Transport {
  int flavour = 0;  // 0: exported only; YDC_TRANSPORT_IPC_DEVICE / YDC_TRANSPORT_IPC_HOST once initialised
  int rank = -1, n_ranks = 0;  // as exported
  size_t bytes = 0;            // two sets of n_ranks slots of 8-byte granules
  uint32_t slot_words = 0;     // payload words of a slot (YDC_TUNE ipc_slot_words, read at every export)
  uint32_t seq = 0;            // exchanges so far (the stamp; never 0)
  MailboxHostSegment own_host;
  MailboxDevBlock own_dev;
  MailboxPeers peers{};
  MailboxPeerMap opened[kMailboxMaxRanks];
  ~MailboxTransport() override { close_peers(); }  // (then the own blocks, device first)

  void close_peers() {
    for (uint32_t q = 0; q < kMailboxMaxRanks; ++q) {
      opened[q].close();
      peers.box[q] = nullptr;
    }
    flavour = 0;
    seq = 0;
  }
  // Rank q's mailbox of the given flavour, from the blob it exported, into peers.box[q].
  int open_peer(ydc_context* c, const MailboxBlob& pb, int q, bool host) {
    const bool same_process = pb.pid == (int32_t)getpid();
    void* dev_ptr = nullptr;
    if (!host) {
      if (!pb.have_device) return fail(c, YDC_ERR_HIP, "rank %d exported no device mailbox", q);
      if (q == rank) {
        dev_ptr = own_dev.p;
      } else if (same_process) {
        dev_ptr = (void*)(uintptr_t)pb.raw_dev;  // a peer inside this process: its own pointer
      } else {
        hipError_t e = hipIpcOpenMemHandle(&dev_ptr, pb.handle, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
          (void)hipGetLastError();
          return fail(c, YDC_ERR_HIP, "hipIpcOpenMemHandle(rank %d): %s", q, hipGetErrorString(e));
        }
        opened[q].dev = dev_ptr;
      }
    } else {
      if (!pb.have_host) return fail(c, YDC_ERR_HIP, "rank %d exported no host mailbox", q);
      void* m = nullptr;
      if (q == rank) {
        m = own_host.p;
      } else if (same_process) {
        m = (void*)(uintptr_t)pb.raw_host;
      } else {
        int fd = shm_open(pb.shm_name, O_RDWR, 0600);
        if (fd < 0) return fail(c, YDC_ERR_HIP, "shm_open(%s) of rank %d failed", pb.shm_name, q);
        m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        (void)close(fd);
        if (m == MAP_FAILED) return fail(c, YDC_ERR_HIP, "mmap of rank %d's mailbox failed", q);
        hipError_t e = hipHostRegister(m, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
        if (e != hipSuccess) {
          (void)hipGetLastError();
          (void)munmap(m, bytes);
          return fail(c, YDC_ERR_HIP, "hipHostRegister of rank %d's mailbox: %s", q, hipGetErrorString(e));
        }
        opened[q].host = m;
        opened[q].bytes = bytes;
      }
      HIP_TRY(c, hipHostGetDevicePointer(&dev_ptr, m, 0));
    }
    peers.box[q] = (unsigned long long*)dev_ptr;
    return YDC_OK;
  }

  int kind() const override { return flavour; }
  int gather(ydc_context* c, const void* send, void* recv, size_t nbytes) override {
    if (n_ranks == 1) return solo_gather(c, send, recv, nbytes);
    if (nbytes % 4) return fail(c, YDC_ERR_INVALID_ARGUMENT, "mailbox exchange of %zu bytes", nbytes);
    const uint32_t words = (uint32_t)(nbytes / 4), G = (uint32_t)n_ranks;
    for (uint32_t off = 0; off < words; off += slot_words) {
      const uint32_t n = std::min(slot_words, words - off);
      if (++seq == 0) ++seq;
      const uint32_t bpp = std::min(16u, std::max(1u, ceil_div(n, 1024)));
      YDC_LAUNCH(c, "k_mailbox_all_gather", k_mailbox_all_gather, dim3(G * bpp), dim3(256), 0, c->stream, peers,
                 (uint32_t)rank, G, (const uint32_t*)send + off, (uint32_t*)recv + off, n, words, slot_words,
                 seq & 1u, seq, bpp, c->group.mailbox_timeout_ticks, c->d_prm.p);
    }
    return YDC_OK;
  }
  int settled(ydc_context* c) override {
    uint32_t late = 0;
    HIP_TRY(c, hipMemcpyAsync(&late, &c->d_prm.p->exchange_timeout, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return late ? late_peer(c) : YDC_OK;
  }
};

// Leaves the group: the transport gives back what it took, the workspace goes as a whole.
void group_release(ydc_context* c) {
  auto& g = c->group;
  g.via.reset();
  g.ws = ydc_context::Group::Workspace{};
  g.n_ranks = 0;
}

// What every entry point of the group does first: the context's device, the resident kernel out
// of the way (the registry leaves its registers), and — except for a batch, whose stream is in
// order already — the stream drained and the present group left. ydc_group_init_ipc alone keeps
// what is there: it completes the mailbox ydc_group_ipc_export made.
enum class GroupKeep { kNothing, kExport, kGroup };
int group_enter(ydc_context* c, GroupKeep keep) {
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);
  if (keep == GroupKeep::kGroup) return YDC_OK;
  if (c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (keep == GroupKeep::kNothing) group_release(c);
  return YDC_OK;
}

}  // namespace

extern "C" {

int ydc_group_unique_id(void* out_id128) {
  if (!out_id128) return YDC_ERR_INVALID_ARGUMENT;
  static_assert(sizeof(ncclUniqueId) == 128, "ydc_group_unique_id hands out 128 bytes");
  RcclApi api;  // the handle stays open: ydc_group_init reuses the loaded library
  std::string rccl_err;
  if (!api.open(&rccl_err)) {
    set_create_error(rccl_err);
    return YDC_ERR_HIP;
  }
  if (!api.get_unique_id) {
    set_create_error("librccl has no ncclGetUniqueId");
    return YDC_ERR_HIP;
  }
  ncclUniqueId id;
  if (api.get_unique_id(&id) != ncclSuccess) {
    set_create_error("ncclGetUniqueId failed");
    return YDC_ERR_HIP;
  }
  std::memcpy(out_id128, &id, sizeof(id));
  return YDC_OK;
}

int ydc_group_init(ydc_context* c, const void* id128, int rank, int n_ranks) {
  if (!c || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = group_enter(c, GroupKeep::kNothing)) return rc;
  auto t = std::make_unique<RcclTransport>();
  std::string err;
  if (!t->api.open(&err)) return fail(c, YDC_ERR_HIP, "%s", err.c_str());
  if (!t->api.comm_init_rank || !t->api.all_gather || !t->api.comm_destroy)
    return fail(c, YDC_ERR_HIP, "librccl lacks ncclCommInitRank / ncclAllGather / ncclCommDestroy");
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  ncclResult_t r = t->api.comm_init_rank(&t->comm, n_ranks, id, rank);
  if (r != ncclSuccess) {
    t->comm = nullptr;
    return fail(c, YDC_ERR_HIP, "ncclCommInitRank(rank %d of %d): %s", rank, n_ranks, t->api.text(r));
  }
  t->solo = n_ranks == 1;
  c->group.via = std::move(t);
  c->group.rank = rank;
  c->group.n_ranks = n_ranks;
  return YDC_OK;
}

int ydc_group_init_local(ydc_context** ctxs, int n) {
  if (!ctxs || n < 1) return YDC_ERR_INVALID_ARGUMENT;
  for (int r = 0; r < n; ++r)
    if (!ctxs[r]) return YDC_ERR_INVALID_ARGUMENT;
  auto hub = std::make_shared<LocalHub>();
  hub->n = n;
  hub->send.assign(n, nullptr);
  for (int r = 0; r < n; ++r) {
    if (int rc = group_enter(ctxs[r], GroupKeep::kNothing)) return rc;
    auto t = std::make_unique<LocalHubTransport>();
    t->hub = hub;
    t->rank = r;
    ctxs[r]->group.via = std::move(t);
    ctxs[r]->group.rank = r;
    ctxs[r]->group.n_ranks = n;
  }
  return YDC_OK;
}

int ydc_group_ipc_export(ydc_context* c, int rank, int n_ranks, void* out_handle) {
  if (!c || !out_handle || n_ranks < 1 || n_ranks > (int)kMailboxMaxRanks || rank < 0 || rank >= n_ranks)
    return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = group_enter(c, GroupKeep::kNothing)) return rc;
  auto box = std::make_unique<MailboxTransport>();
  // Slots of 64 KB of payload (a configs[3] registry's slot deltas: 16k servants x 4 B) unless
  // tuned; two sets of n_ranks slots of 8-byte granules.
  box->slot_words = 16384;
  if (const char* e = tune_value("ipc_slot_words")) box->slot_words = (uint32_t)std::max(64, atoi(e));
  if (const char* e = tune_value("ipc_timeout_ms"))
    c->group.mailbox_timeout_ticks = (unsigned long long)std::max(1, atoi(e)) * 100000ull;  // 100 MHz wall clock
  box->bytes = (size_t)2 * n_ranks * box->slot_words * 8;
  box->rank = rank;
  box->n_ranks = n_ranks;
  const char* coarse = tune_value("ipc_coarse");
  HIP_TRY(c, box->own_dev.create(box->bytes, coarse && atoi(coarse)));
  box->own_host.create(c, box->bytes);
  MailboxBlob blob{};
  blob.magic = kMailboxMagic;
  blob.abi = ydc_abi_version();
  blob.rank = rank;
  blob.n_ranks = n_ranks;
  blob.slot_words = box->slot_words;
  blob.device = c->device;
  blob.pid = (int32_t)getpid();
  blob.bytes = box->bytes;
  blob.have_device = box->own_dev.p != nullptr;
  blob.device_fine = box->own_dev.fine;
  blob.raw_dev = (uint64_t)(uintptr_t)box->own_dev.p;
  if (box->own_dev.have_handle) blob.handle = box->own_dev.handle;
  blob.have_host = box->own_host.p != nullptr;
  blob.raw_host = (uint64_t)(uintptr_t)box->own_host.p;
  std::memcpy(blob.shm_name, box->own_host.name, sizeof(blob.shm_name));
  if (!blob.have_device && !blob.have_host)
    return fail(c, YDC_ERR_HIP, "neither a device nor a host mailbox could be set up");
  c->group.via = std::move(box);  // (n_ranks stays 0: not in a group before ydc_group_init_ipc)
  std::memset(out_handle, 0, YDC_IPC_HANDLE_BYTES);
  std::memcpy(out_handle, &blob, sizeof(blob));
  return YDC_OK;
}

int ydc_group_init_ipc(ydc_context* c, const void* handles, int rank, int n_ranks, int transport) {
  if (!c || !handles || n_ranks < 1 || n_ranks > (int)kMailboxMaxRanks || rank < 0 || rank >= n_ranks)
    return YDC_ERR_INVALID_ARGUMENT;
  if (transport != YDC_TRANSPORT_IPC_DEVICE && transport != YDC_TRANSPORT_IPC_HOST)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "transport %d is not a mailbox transport", transport);
  auto& g = c->group;
  auto* box = dynamic_cast<MailboxTransport*>(g.via.get());
  if (!box || box->n_ranks != n_ranks || box->rank != rank)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_group_ipc_export(rank %d of %d) first", rank, n_ranks);
  if (int rc = group_enter(c, GroupKeep::kExport)) return rc;
  // (a second attempt with the other flavour: drop what the first one mapped; not in a group
  // until every peer is)
  g.n_ranks = 0;
  box->close_peers();
  for (int q = 0; q < n_ranks; ++q) {
    MailboxBlob pb;
    std::memcpy(&pb, (const char*)handles + (size_t)q * YDC_IPC_HANDLE_BYTES, sizeof(pb));
    if (pb.magic != kMailboxMagic || pb.rank != q || pb.n_ranks != n_ranks || pb.slot_words != box->slot_words ||
        pb.bytes != box->bytes)
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "handle %d does not describe rank %d of %d with %u-word slots", q,
                  q, n_ranks, box->slot_words);
    if (int rc = box->open_peer(c, pb, q, transport == YDC_TRANSPORT_IPC_HOST)) return rc;
  }
  box->flavour = transport;
  g.rank = rank;
  g.n_ranks = n_ranks;
  return YDC_OK;
}

int ydc_group_transport(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  return c->group.n_ranks < 1 ? YDC_TRANSPORT_NONE : c->group.via->kind();
}

int ydc_group_size(ydc_context* c, int* out_ranks, int* out_is_rccl) {
  if (!c || !out_ranks) return YDC_ERR_INVALID_ARGUMENT;
  auto& g = c->group;
  *out_ranks = g.n_ranks;
  if (out_is_rccl) *out_is_rccl = g.n_ranks >= 1 && g.via->kind() == YDC_TRANSPORT_RCCL;
  return g.n_ranks >= 1 ? g.via->count(c, out_ranks) : YDC_OK;
}

int ydc_group_destroy(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (group_enter(c, GroupKeep::kNothing)) group_release(c);  // (whatever the device says, the group goes)
  return YDC_OK;
}

}  // extern "C"

namespace {

// One ydc_dispatch_sharded call: this rank's slice and where its results go (device addresses).
struct ShardCall {
  const ydc_task_soa* tk = nullptr;
  uint32_t N = 0, flags = 0;
  uint32_t* out_idx = nullptr;
  double* out_util = nullptr;
  uint32_t* out_running = nullptr;
};

// One attempt at the batch: the plan it runs with and how far it has got. The sizes are those
// of the registry and the group, the same on every rank.
struct ShardAttempt {
  uint32_t G = 0, C = 0, S = 0, K = 0;
  uint32_t P = 0;   // counts are exchanged per independent part of the registry
  uint32_t MS = 0;  // words of a rank's k_rank_meta record
  size_t rec = 0;   // ClassStates a rank publishes per pass
  BatchPlan p;
  bool windowed = false;
  uint32_t launched = 0;  // matching passes enqueued so far
};

// What the host finds behind a group of passes and its tail.
struct ShardOutcome {
  enum What { kSettled, kGoOn, kMissed, kFailed } what = kFailed;
  uint32_t rounds = 0;  // kSettled: passes up to the first in which no rank changed anything
  int rc = YDC_OK;      // kFailed
};

// Registries the sharded matching does not take (> 256 classes: thread-per-chunk path): every
// rank gathers the whole batch, places it redundantly with the single-GPU pipeline — identical
// on all ranks — and keeps its own slice of the placement.
int sharded_replicated(ydc_context* c, const ShardCall& call) {
  auto& g = c->group;
  auto& w = g.ws;
  const uint32_t G = (uint32_t)g.n_ranks, N = call.N;
  HIP_TRY(c, w.d_totals.reserve(G + 1));
  HIP_TRY(c, hipMemcpyAsync(w.d_totals.p + G, &N, 4, hipMemcpyHostToDevice, c->stream));
  if (int rc = g.via->gather(c, w.d_totals.p + G, w.d_totals.p, 4)) return rc;
  std::vector<uint32_t> sizes(G);
  HIP_TRY(c, hipMemcpyAsync(sizes.data(), w.d_totals.p, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
  if (int rc = g.via->settled(c)) return rc;  // (a late peer's size would read as 0)
  const ShardSlices sl = shard_slices(sizes.data(), G, (uint32_t)g.rank);
  HIP_TRY(c, w.d_pad.reserve(sl.max_n));
  HIP_TRY(c, w.d_gather.reserve((size_t)sl.max_n * G));
  for (auto& col : w.d_all) HIP_TRY(c, col.reserve(sl.total));
  HIP_TRY(c, w.d_all_idx.reserve(sl.total));
  if (call.out_util) HIP_TRY(c, w.d_all_util.reserve(sl.total));
  const uint32_t* cols[3] = {N ? call.tk->env_id : nullptr, N ? call.tk->min_version : nullptr,
                             N ? call.tk->requestor_ip : nullptr};
  for (int k = 0; k < 3; ++k) {
    if (N) HIP_TRY(c, hipMemcpyAsync(w.d_pad.p, cols[k], (size_t)N * 4, hipMemcpyDeviceToDevice, c->stream));
    if (int rc = g.via->gather(c, w.d_pad.p, w.d_gather.p, (size_t)sl.max_n * 4)) return rc;
    uint32_t off = 0;
    for (uint32_t r = 0; r < G; ++r) {
      if (sizes[r])
        HIP_TRY(c, hipMemcpyAsync(w.d_all[k].p + off, w.d_gather.p + (size_t)r * sl.max_n, (size_t)sizes[r] * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
      off += sizes[r];
    }
  }
  // (... and a late peer's columns as zeros: nothing is placed, let alone committed, on them)
  if (int rc = g.via->settled(c)) return rc;
  ydc_task_soa all{w.d_all[0].p, w.d_all[1].p, w.d_all[2].p};
  if (int rc = ydc_dispatch_device(c, &all, sl.total, call.flags, w.d_all_idx.p,
                                   call.out_util ? w.d_all_util.p : nullptr, call.out_running))
    return rc;
  if (N && call.out_idx)
    HIP_TRY(c, hipMemcpyAsync(call.out_idx, w.d_all_idx.p + sl.my_off, (size_t)N * 4, hipMemcpyDeviceToDevice,
                              c->stream));
  if (N && call.out_util)
    HIP_TRY(c, hipMemcpyAsync(call.out_util, w.d_all_util.p + sl.my_off, (size_t)N * 8, hipMemcpyDeviceToDevice,
                              c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // Stats describe the whole batch in this mode; report this rank's share of the grants.
  c->stats.n_tasks = N;
  g.passes = c->stats.rounds;
  return YDC_OK;
}

// The sizes of the batch and the workspace every attempt uses.
int shard_prepare(ydc_context* c, const BatchPlan& full_plan, ShardAttempt* a) {
  auto& g = c->group;
  auto& w = g.ws;
  a->G = (uint32_t)g.n_ranks, a->C = full_plan.C, a->S = full_plan.S, a->K = full_plan.K;
  a->rec = (size_t)a->C + 1;
  a->P = c->n_parts;
  a->MS = a->P + 1;
  HIP_TRY(c, w.d_totals.reserve((size_t)a->G * a->MS));
  HIP_TRY(c, w.d_meta.reserve(a->MS));
  HIP_TRY(c, w.d_bound_local.reserve(a->C ? a->C : 1));
  HIP_TRY(c, w.d_base.reserve(a->P));
  HIP_TRY(c, w.d_send.reserve(a->rec));
  HIP_TRY(c, w.d_bounds.reserve(a->rec * a->G));
  HIP_TRY(c, w.d_delta.reserve(a->S));
  HIP_TRY(c, w.d_deltas.reserve((size_t)a->S * a->G));
  HIP_TRY(c, g.h_bounds.reserve(a->rec * a->G * sizeof(ClassState), hipHostMallocDefault));
  return YDC_OK;
}

// The plan of one attempt, from the full or the window plan: this rank's place in the group
// and, for a window, its size (shard_plan.h) and its buffers.
int shard_plan_attempt(ydc_context* c, const ShardCall& call, const BatchPlan& plan, ShardAttempt* a) {
  auto& g = c->group;
  auto& w = g.ws;
  BatchPlan& p = a->p;
  p = plan;
  a->launched = 0;
  p.mb.has_successor = g.rank + 1 < g.n_ranks ? 1u : 0u;
  p.zone = false;  // (the walk of the tier's end is a single-context thing: zone_guess.h)
  p.mb.zone_box = nullptr;
  if (a->windowed) {
    const ShardWindow win = shard_window(call.N, g.margin_scale, c->opt_shard_margin, plan.slot_bound, kSortThreads);
    p.win = true;
    p.win_margin = win.win_margin;
    p.slot_bound = win.slot_bound;
    p.sort_items = win.sort_items;
    p.n_tiles = win.n_tiles;
    if (p.mb.tile_tab) {  // (the window's own tiles: ranks are registry-wide, rank_offset apart)
      p.mb.tile_tab_tiles = p.n_tiles;
      p.mb.tile_tab_elems = kSortThreads * p.sort_items;
    }
    HIP_TRY(c, w.d_cum.reserve(kWindowThresholds + 1));
    HIP_TRY(c, w.d_r_first.reserve(a->S));
    HIP_TRY(c, w.d_lbase.reserve((size_t)a->S + 1));
    HIP_TRY(c, w.d_cls_begin_glob.reserve((size_t)a->C + 1));
    HIP_TRY(c, w.d_shift.reserve(a->C));
    HIP_TRY(c, w.d_winrec.reserve((size_t)2 * a->C));
    HIP_TRY(c, w.d_winall.reserve((size_t)2 * a->C * a->G));
    ++g.windowed_batches;
  }
  // The chunks of this rank continue those of the nearest rank below that has requests
  // (k_global_flag / k_boundary_in copy its end state — sharded sort: translated into this
  // rank's local list positions — into d_bound_local after every exchange).
  p.mb.boundary_in = g.rank == 0 ? nullptr : w.d_bound_local.p;
  return YDC_OK;
}

// Front: the slot order (full: scan, generation and sort of the whole registry; windowed:
// classification, the counts' exchange, key counts, this rank's window, the windows' exchange,
// generation and sort of the window) and the chunks' level guesses from the gathered counts.
int shard_front(ydc_context* c, const ShardCall& call, ShardAttempt* a) {
  auto& g = c->group;
  auto& w = g.ws;
  BatchPlan& p = a->p;
  const uint32_t N = call.N, G = a->G, C = a->C, K = a->K, P = a->P, MS = a->MS;
  hipStream_t st = c->stream;
  DeviceParams* prm = c->d_prm.p;
  if (!a->windowed) {
    if (int rc = enqueue_front_a(c, p, call.tk)) return rc;
  } else {
    enqueue_scan(c, p, w.d_cls_begin_glob.p);
    enqueue_gen(c, p, call.tk, false, true);  // classification only
    if (N) {
      PrefixArgs pa{c->d_chunk_consuming.p, K, c->d_before.p, P, 0u, 0u};
      YDC_LAUNCH(c, "k_chunk_prefix", k_chunk_prefix, dim3(1), dim3(1024), 0, st, pa, prm);
    }
  }
  if (!N) HIP_TRY(c, hipMemsetAsync(c->d_before.p, 0, (size_t)4 * P, st));  // totals row of K == 0
  // Level guesses count the consuming requests of the ranks before this one; a rank without
  // requests is skipped by its successor (k_rank_meta: counts per part + number of requests).
  hipLaunchKernelGGL(k_rank_meta, dim3(1), dim3(64), 0, st, c->d_before.p + (size_t)K * P, P, N, w.d_meta.p);
  if (int rc = g.via->gather(c, w.d_meta.p, w.d_totals.p, (size_t)4 * MS)) return rc;
  if (a->windowed) {
    const uint32_t log_t = 7;  // kWindowThresholds == 128
    static_assert(kWindowThresholds == 128, "threshold shift");
    const uint32_t shift = c->kf.key_bits > log_t ? c->kf.key_bits - log_t : 0;
    YDC_LAUNCH(c, "k_key_count", k_key_count, dim3(kWindowThresholds - 1), dim3(256), 0, st, p.sv, c->kf.cap_bits,
               shift, w.d_cum.p);
    WindowArgs wa{w.d_cum.p, c->kf.cap_bits, shift, w.d_totals.p, MS, (uint32_t)g.rank, G, p.win_margin,
                  p.slot_bound, c->d_slot_base.p, w.d_cls_begin_glob.p, C, w.d_r_first.p,
                  w.d_lbase.p, c->d_cls_begin.p, w.d_shift.p, w.d_winrec.p};
    YDC_LAUNCH(c, "k_window", k_window, dim3(1), dim3(1024), (size_t)2 * C * 4, st, p.sv, wa, prm);
    if (int rc = g.via->gather(c, w.d_winrec.p, w.d_winall.p, (size_t)2 * C * 4)) return rc;
    enqueue_gen(c, p, call.tk, true, false);  // the window's slots
    if (int rc = enqueue_sort(c, p, false)) return rc;
  }
  if (p.wave_path && p.W == 1 && c->opt_own_guess) {
    // Pass 0 works the guesses out itself, from the gathered counts.
    p.mb.before = c->d_before.p;
    p.mb.base_totals = w.d_totals.p;
    p.mb.base_rank = (uint32_t)g.rank;
    p.mb.base_stride = MS;
    if (int rc = enqueue_front_b(c, p, nullptr)) return rc;
  } else {
    hipLaunchKernelGGL(k_rank_base, dim3(1), dim3(64), 0, st, w.d_totals.p, (uint32_t)g.rank, P, MS, w.d_base.p);
    if (int rc = enqueue_front_b(c, p, w.d_base.p)) return rc;
  }
  mark(c, 6);
  return YDC_OK;
}

// Matching passes [first, first + count), pre-launched like on one GPU: after every pass the
// ranks all-gather (end state of the last chunk, "changed an end state" flag); k_global_flag /
// k_boundary_in turn the flags into one global flag per pass, which gates the following passes
// on every rank alike.
int shard_passes(ydc_context* c, ShardAttempt* a, uint32_t first, uint32_t count) {
  auto& g = c->group;
  auto& w = g.ws;
  const BatchPlan& p = a->p;
  const uint32_t G = a->G, C = a->C, MS = a->MS, rec = (uint32_t)a->rec;
  hipStream_t st = c->stream;
  DeviceParams* prm = c->d_prm.p;
  for (uint32_t r = first; r < first + count; ++r) {
    if (first) {  // (the first group's counter slots were cleared with the batch)
      HIP_TRY(c, hipMemsetAsync(&prm->n_changed[r & 63], 0, 4, st));
      HIP_TRY(c, hipMemsetAsync(&prm->n_sampled[r & 63], 0, 4, st));
    }
    if (p.wave_path) enqueue_pass(c, p, r, 1u);
    hipLaunchKernelGGL(k_pack_boundary, dim3(ceil_div(rec, 256)), dim3(256), 0, st, p.L, c->d_endst.p,
                       p.wave_path ? a->K : 0u, p.mb.boundary_in, prm, r, w.d_send.p,
                       a->windowed ? w.d_shift.p : nullptr);
    if (int rc = g.via->gather(c, w.d_send.p, w.d_bounds.p, a->rec * sizeof(ClassState))) return rc;
    if (a->windowed) {
      hipLaunchKernelGGL(k_boundary_in, dim3(ceil_div(C, 256)), dim3(256), 0, st, w.d_bounds.p, rec, C, G,
                         (uint32_t)g.rank, r, w.d_winall.p, w.d_cls_begin_glob.p, w.d_totals.p, MS, w.d_shift.p,
                         w.d_bound_local.p, prm);
    } else {
      hipLaunchKernelGGL(k_global_flag, dim3(std::max(1u, ceil_div(C, 256))), dim3(256), 0, st, w.d_bounds.p, rec,
                         C, G, (uint32_t)g.rank, r, w.d_totals.p, MS, c->d_cls_begin.p, w.d_bound_local.p, prm);
    }
  }
  a->launched = first + count;
  return YDC_OK;
}

// The tail behind a group of passes, gated on the device by the last pass's global flag (the
// same on every rank): placement of this rank's slice, then the global running_tasks from
// everybody's slot deltas. Not converged yet (or a window missed): the deltas are zero and
// nothing changes.
int shard_tail(ydc_context* c, const ShardCall& call, const ShardAttempt& a) {
  auto& g = c->group;
  auto& w = g.ws;
  // (no COMMIT and no running_tasks from the finalise: k_sum_deltas does both, below)
  BatchCall slice;
  slice.out_idx = call.out_idx;
  slice.out_util = call.out_util;
  if (int rc = enqueue_finalize(c, a.p, slice, (a.launched - 1) & 63, w.d_delta.p, a.p.mb.boundary_in)) return rc;
  if (a.S) {
    if (int rc = g.via->gather(c, w.d_delta.p, w.d_deltas.p, (size_t)a.S * 4)) return rc;
    hipLaunchKernelGGL(k_sum_deltas, dim3(ceil_div(a.S, 256)), dim3(256), 0, c->stream, c->d_running.p,
                       w.d_deltas.p, a.S, a.G, c->d_running_out.p, call.out_running,
                       (call.flags & YDC_DISPATCH_COMMIT) ? c->d_running.p : nullptr, c->d_prm.p);
  }
  mark(c, 7);
  return YDC_OK;
}

// debug_sim: what the passes [first, launched) left, and on rank 0 every rank's record of the
// last pass (registry-wide positions).
void shard_debug_dump(ydc_context* c, const ShardAttempt& a, uint32_t first) {
  auto& g = c->group;
  const uint32_t G = a.G, C = a.C;
  const size_t rec = a.rec;
  fprintf(stderr, "[ydc sharded] rank %d/%u windowed %d launched %u n_slots %u rank_offset %u miss %u changed:",
          g.rank, G, (int)a.windowed, a.launched, c->h_prm->n_slots, c->h_prm->rank_offset, c->h_prm->window_miss);
  for (uint32_t r = first; r < a.launched; ++r) fprintf(stderr, " %u", c->h_prm->n_changed[r & 63]);
  fprintf(stderr, "\n");
  if (g.rank != 0 || a.launched > 30) return;
  (void)hipMemcpy(g.h_bounds, g.ws.d_bounds.p, rec * G * sizeof(ClassState), hipMemcpyDeviceToHost);
  for (uint32_t q = 0; q < G; ++q) {
    fprintf(stderr, "   rank %u flag %u:", q, g.h_bounds[q * rec + C].cursor);
    for (uint32_t k = 0; k < std::min(C, 8u); ++k)
      fprintf(stderr, " (%u,%u,%x)", g.h_bounds[q * rec + k].cursor, g.h_bounds[q * rec + k].lo,
              g.h_bounds[q * rec + k].hown_lo);
    fprintf(stderr, "\n");
  }
}

// Reads DeviceParams back behind the tail of the passes [first, launched) and says what they
// came to — the same verdict on every rank, from flags every rank sees alike.
ShardOutcome shard_outcome(ydc_context* c, const ShardAttempt& a, uint32_t first) {
  ShardOutcome o;
  auto failed = [&](int rc) {
    o.what = ShardOutcome::kFailed;
    o.rc = rc;
    return o;
  };
  auto readback = [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(c->h_prm, c->d_prm.p, sizeof(DeviceParams), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return YDC_OK;
  };
  if (int rc = readback()) return failed(rc);
  if (c->debug_sim) shard_debug_dump(c, a, first);
  if (c->h_prm->overflow) return failed(fail(c, YDC_ERR_CAPACITY, "slot workspace overflow on some rank"));
  if (c->h_prm->exchange_timeout) return failed(late_peer(c));
  // (Belt and braces: a sharded sort that has not settled after 256 passes — the same count
  // on every rank — is treated like a missed window.)
  if (c->h_prm->window_miss || (a.windowed && a.launched >= 256)) {
    o.what = ShardOutcome::kMissed;
  } else if (c->h_prm->n_changed[(a.launched - 1) & 63] == 0) {
    o.what = ShardOutcome::kSettled;
    o.rounds = shard_rounds(c->h_prm->n_changed, first, a.launched - first);
  } else {
    o.what = ShardOutcome::kGoOn;
  }
  return o;
}

}  // namespace

extern "C" {

int ydc_dispatch_sharded(ydc_context* c, const ydc_task_soa* tk, uint32_t N, uint32_t flags,
                         uint32_t* d_out_idx, double* d_out_util, uint32_t* d_out_running) {
  if (!c || (N && !tk)) return YDC_ERR_INVALID_ARGUMENT;
  auto& g = c->group;
  if (g.n_ranks < 1) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_group_init first");
  if (int rc = group_enter(c, GroupKeep::kGroup)) return rc;
  const ShardCall call{tk, N, flags, d_out_idx, d_out_util, d_out_running};
  BatchPlan full_plan, win_plan;
  if (int rc = plan_batch(c, N, &full_plan)) return rc;
  if (full_plan.use_generic) return sharded_replicated(c, call);
  ShardAttempt a;
  if (int rc = shard_prepare(c, full_plan, &a)) return rc;
  // Sharded sort (kernels.h: k_key_count / k_window): this rank generates and
  // sorts only the key window its rank range can reach. Taken for integer keys, one part, a
  // servant per host, 2 .. 256 classes; anything else — and any batch whose window turns out
  // too small (window_miss, the same verdict on every rank) — runs with the full sort on
  // every rank. YDC_SHARD_SORT=0 switches it off.
  // (Decided from the registry alone — every rank must take the same branch, whatever its slice.)
  // A registry small enough for the bin sort is ordered whole on every rank (two launches, no
  // exchange) — cheaper than the key-count / window / radix sequence until the slot count is in
  // the millions; the windows are for the registries the bin sort does not take.
  WindowedInputs wi;
  wi.n_ranks = a.G, wi.n_parts = a.P, wi.n_classes = a.C;
  wi.shard_sort = c->opt_shard_sort, wi.exact_keys = c->kf.exact;
  wi.use_generic = full_plan.use_generic, wi.any_shared = full_plan.any_shared;
  wi.binsort = full_plan.binsort, wi.group_binsort = c->opt_group_binsort;
  a.windowed = shard_windowed(wi);
  if (a.windowed)
    if (int rc = plan_batch(c, N, &win_plan, true)) return rc;
  // An attempt is a front and groups of passes, each with its tail, until one settles. The host
  // looks at the outcome once per group.
  ShardOutcome o;
  for (;;) {
    if (int rc = shard_plan_attempt(c, call, a.windowed ? win_plan : full_plan, &a)) return rc;
    if (int rc = shard_front(c, call, &a)) return rc;
    do {
      const uint32_t first = a.launched;
      if (int rc = shard_passes(c, &a, first, shard_pass_group(first, g.pass_hint))) return rc;
      if (int rc = shard_tail(c, call, a)) return rc;
      o = shard_outcome(c, a, first);
      // More than 200000 passes: given up. (Worst case one chunk per pass becomes final; K
      // differs per rank, so bound it loosely.)
      if (o.what == ShardOutcome::kGoOn && a.launched > 200000u) return fail(c, YDC_ERR_NOT_CONVERGED, "no fixpoint");
    } while (o.what == ShardOutcome::kGoOn);
    if (o.what == ShardOutcome::kFailed) return o.rc;
    if (o.what == ShardOutcome::kSettled) break;
    if (!a.windowed && a.p.binsort) {
      // A bin of the bin sort overflowed (bin_sort.h; the registry decides, so every rank met
      // the same): once more with the radix pipeline, which then stays.
      note_bin_overflow(c);
      if (int rc = plan_batch(c, N, &full_plan)) return rc;
      continue;
    }
    if (!a.windowed) return fail(c, YDC_ERR_NOT_CONVERGED, "window miss flagged without a window");
    // Some rank's window did not cover what its requests reached, or 256 windowed passes did
    // not settle (every rank saw the same): once more with the full sort everywhere, and wider
    // margins from now on.
    ++g.window_misses;
    g.margin_scale = shard_margin_after_miss(g.margin_scale);
    a.windowed = false;
  }
  g.pass_hint = g.passes = o.rounds;

  fill_stats(c, a.p, o.rounds);
  if (c->profiling) collect_kernel_profile(c);
  return YDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Streaming mode (BASELINE.json configs[4]): a tick is
//   n_upd heartbeats of known servants  (KeepServantAlive, task_dispatcher.cc:195-201)
//   n_rel released grants               (FreeTask's --running_tasks, :181)
//   n_tasks requests, committed         (WaitForStartingNewTask x n, timeout == now)
// in this order. The whole step — staging copies, row scatter, release, the batch
// pipeline with a fixed number of pre-launched matching passes, the gated finalise and
// the result copy — is captured once into a hipGraph and replayed per tick. Lists shorter
// than the captured capacity are padded with no-ops (index 0xFFFFFFFF; requests for a
// digest nobody has), which changes nothing for the real entries. Heartbeats that change
// the registry's structure (new servant, other environments / version / host / capacity
// bound) are applied eagerly and the step is captured again.
// ---------------------------------------------------------------------------
namespace {

void stream_drop_graphs(ydc_context::Stream& sm) {
  if (sm.exec) (void)hipGraphExecDestroy(sm.exec);
  if (sm.graph) (void)hipGraphDestroy(sm.graph);
  if (sm.exec_b) (void)hipGraphExecDestroy(sm.exec_b);
  if (sm.graph_b) (void)hipGraphDestroy(sm.graph_b);
  sm.exec = sm.exec_b = nullptr;
  sm.graph = sm.graph_b = nullptr;
}

void stream_release(ydc_context::Stream& sm) {
  stream_drop_graphs(sm);
  sm = ydc_context::Stream{};  // (frees every buffer the stream owns: ydc_stream_end discards W)
}

void stream_release(ydc_context* c) { stream_release(c->stream_mode); }

// Offset of the next 256 B aligned section of an arena that is `*off` bytes long so far.
size_t section(size_t* off, size_t bytes) {
  const size_t at = *off;
  *off += (std::max<size_t>(bytes, 16) + 255) & ~(size_t)255;
  return at;
}

// Requests one streaming batch places: the new ones, behind W's region in waiting mode; the
// expanded rows in rpc mode.
uint32_t stream_batch_n(const ydc_context::Stream& sm) {
  return sm.rpc() ? sm.caps.max_rows : sm.caps.max_tasks + sm.caps.max_waiting;
}

// The tick's heartbeats and frees applied to the registry's device columns, from the arena as
// `a` sees it (in place, or its device mirror).
void enqueue_apply_tick(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  if (!(sm.caps.max_updates + sm.caps.max_releases)) return;
  const uint32_t upd_blocks = ceil_div(sm.caps.max_updates, 256);
  hipLaunchKernelGGL(k_apply_tick, dim3(upd_blocks + ceil_div(sm.caps.max_releases, 256)), dim3(256), 0, c->stream,
                     a.upd_idx, (ServantRowDev*)a.upd_rows, sm.caps.max_updates, upd_blocks, a.rel, sm.caps.max_releases,
                     c->reg.n, c->d_version.p, c->d_nproc.p, c->d_load.p, c->d_max_tasks.p, c->d_flags.p,
                     c->d_running.p);
}

// Waiting mode: the tick's batch columns from W and the new requests (wait_queue.h), which the
// launch reads from the arena as `a` sees it.
void enqueue_wait_gather(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  const uint32_t N = stream_batch_n(sm);
  YDC_LAUNCH(c, "k_wait_gather", k_wait_gather, dim3(ceil_div(std::max(N, sm.lookback_n), 256)), dim3(256), 0,
             c->stream, sm.wq, sm.wt,
             // (with a quota: the env column in which a refused request is padding — stream_quota.h)
             WaitNew{sm.quota.on ? sm.quota.tk.env : a.env, a.minv, a.ip, a.dl, a.tag, a.now}, sm.caps.max_waiting, N, sm.ws,
             sm.lookback, sm.leased() ? 0u : sm.lookback_n,  // (with leases: k_lease_renew has cleared the words)
             WaitExtra{sm.wl.w_for, sm.wl.t_for, sm.wl.t_for ? a.lexp : nullptr});
}

// RPC mode: W's entries and the new requests expanded into the batch's rows (rpc_stream.h).
void enqueue_rpc_expand(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  const uint32_t P = sm.caps.max_waiting + sm.caps.max_tasks, NR = sm.caps.max_rows;
  // (with a quota: the new requests' counts are the admitted ones, in HBM — stream_quota.h)
  const uint32_t* const nimm = sm.quota.on ? sm.quota.tk.adm_imm : a.nimm;
  const uint32_t* const npre = sm.quota.on ? sm.quota.tk.adm_pre : a.npre;
  YDC_LAUNCH(c, "k_rpc_scan", k_rpc_scan, dim3(ceil_div(P, kRpcTile)), dim3(256), 0, c->stream, sm.rw,
             RpcNew{a.env, a.minv, a.ip, a.dl, a.tag, a.lexp, nimm, npre}, sm.rp, a.lh, sm.caps.max_waiting, P, sm.ws,
             sm.rs, sm.lb_scan, sm.rb.row_start);
  YDC_LAUNCH(c, "k_rpc_expand", k_rpc_expand, dim3(ceil_div(NR, 256)), dim3(256), 0, c->stream, sm.rp, P, NR, sm.rb,
             sm.rs);
}

// The tick's batch columns in HBM, in the context's mode.
void enqueue_stream_gather(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  // With withdrawal: the staged tags' entries of W expire here, in front of the gather that reads W
  // (stream_withdraw.h). In this helper, so once per tick on every route.
  if (sm.max_withdraw) {
    const uint32_t MX = sm.max_withdraw;
    YDC_LAUNCH(c, "k_withdraw_load", k_withdraw_load, dim3(ceil_div(MX, 256)), dim3(256), 0, c->stream, a.wd_tag,
               a.wd_n, MX, sm.withdraw.list);
    YDC_LAUNCH(c, "k_withdraw_mark", k_withdraw_mark, dim3(ceil_div(sm.caps.max_waiting, 256)), dim3(256), 0, c->stream,
               sm.withdraw.list, MX, sm.wq.tag, sm.wq.deadline, sm.ws, sm.caps.max_waiting);
  }
  // With departure: the staged requestors' entries of W expire here as well, behind withdrawal's mark
  // (an entry both name is withdrawal's) and in front of the quota's loads (stream_depart.h).
  if (sm.max_depart) {
    const bool rpc = sm.rpc();
    YDC_LAUNCH(c, "k_depart_mark", k_depart_mark, dim3(ceil_div(sm.caps.max_waiting, 256)), dim3(256), 0, c->stream,
               sm.depart.list, sm.max_depart, rpc ? sm.rw.ip : sm.wq.ip, rpc ? sm.rw.deadline : sm.wq.deadline,
               rpc ? sm.rw.n_imm : nullptr, rpc ? sm.rw.n_pre : nullptr, sm.ws, sm.caps.max_waiting);
  }
  // With a quota: the new requests clipped to their requestors' room, by the loads of L and W as they
  // are here — behind the tick's frees, expiry and the withdrawal's mark (stream_quota.h). In this
  // helper, so once per tick on every route.
  if (sm.quota.on) {
    const auto& q = sm.quota;
    const bool rpc = sm.rpc();
    const uint32_t MT = sm.caps.max_tasks, MW = sm.caps.max_waiting;
    const uint32_t l_blocks = ceil_div(sm.lt.mask + 1, kLeaseTile);
    YDC_LAUNCH(c, "k_quota_claim", k_quota_claim, dim3(ceil_div(std::max(MT, q.tiles), 256)), dim3(256), 0, c->stream,
               a.ip, a.q_n, MT, q.tiles, q.tb, q.tk);
    YDC_LAUNCH(c, "k_quota_loads", k_quota_loads, dim3(l_blocks + ceil_div(MW, 256)), dim3(256), 0, c->stream, sm.lt,
               sm.d_insp_rec.p, l_blocks, rpc ? sm.rw.ip : sm.wq.ip, rpc ? sm.rw.deadline : sm.wq.deadline,
               rpc ? sm.rw.n_imm : nullptr, rpc ? sm.rw.n_pre : nullptr, sm.ws, MW, a.lh, q.tb);
    // With the fair-share level: the pool, what is held and what is asked summed up, the level found and
    // the clip's header of this tick written (stream_fair.h). The clip then reads that header; the
    // override arrays are the settings' own.
    QuotaCaps caps = q.caps;
    if (q.fair_on()) {
      const uint32_t r_blocks = ceil_div(c->reg.n, 256), w_blocks = ceil_div(MW, 256);
      YDC_LAUNCH(c, "k_fair_sums", k_fair_sums, dim3(r_blocks + l_blocks + w_blocks + ceil_div(MT, 256)), dim3(256), 0,
                 c->stream, FairRegistry{c->d_nproc.p, c->d_load.p, c->d_max_tasks.p, c->d_flags.p, c->reg.n}, r_blocks,
                 sm.lt, l_blocks, rpc ? sm.rw.deadline : sm.wq.deadline, rpc ? sm.rw.n_imm : nullptr,
                 rpc ? sm.rw.n_pre : nullptr, sm.ws, MW, w_blocks, a.lh, rpc ? a.nimm : nullptr, rpc ? a.npre : nullptr,
                 a.q_n, MT, q.tk, q.tb, q.fair);
      YDC_LAUNCH(c, "k_fair_level", k_fair_level, dim3(1), dim3(kFairThreads), 0, c->stream, q.tb, q.caps, q.fair, a.lh);
      caps.hdr = q.fair.hdr;
    }
    YDC_LAUNCH(c, "k_quota_clip", k_quota_clip, dim3(q.tiles), dim3(256), 0, c->stream, a.ip, a.env,
               rpc ? a.nimm : nullptr, rpc ? a.npre : nullptr, a.q_n, MT, q.tb, caps, q.tk);
  }
  if (sm.rpc()) enqueue_rpc_expand(c, a);
  else enqueue_wait_gather(c, a);
}

// ... and behind the batch: new W, resolved list, the new requests' answers. prm: gated on the
// batch having become final (the captured step); NULL: the host has just placed it itself.
void enqueue_wait_compact(ydc_context* c, const int64_t* now, const DeviceParams* prm, uint32_t check_slot) {
  auto& sm = c->stream_mode;
  const uint32_t N = stream_batch_n(sm);
  YDC_LAUNCH(c, "k_wait_compact", k_wait_compact, dim3(ceil_div(N, kWaitTile)), dim3(256), 0, c->stream, sm.wt,
             sm.wt_out, now, sm.caps.max_waiting, N, sm.wq, sm.ws, sm.lookback, sm.z_out, sm.z_res_tag,
             sm.z_res_idx, sm.z_wout, prm, check_slot);
}

LeaseIn lease_in(const TickArena& a) {
  return LeaseIn{a.lh, a.ren_id, a.ren_exp, a.free_id, a.rep_srv, a.rep_off, a.rep_id, a.lexp};
}

// Leased mode, in front of the batch: renewals, frees by id, report marks, expiry + sweep
// (lease_table.h), reading the tick from the arena as `a` sees it.
void enqueue_lease_pre(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  const ydc_stream_caps& k = sm.caps;
  const LeaseIn in = lease_in(a);
  const uint32_t S = c->reg.n;
  const uint32_t ren_blocks = ceil_div(k.max_renewals, 256), rep_blocks = ceil_div(k.max_reports, 256);
  // With usage: L and W as the previous tick left them charged for the quanta since then, before anything
  // below changes them (stream_usage.h). Here for the reason the book's pass is here: once per tick on
  // every path.
  if (sm.usage.on) {
    const auto& u = sm.usage;
    const bool rpc = sm.rpc(), with_w = sm.waiting();
    const uint32_t l_blocks = ceil_div(sm.lt.mask + 1, kLeaseTile);
    const uint32_t w_blocks = with_w ? std::min(ceil_div(k.max_waiting, 256), kUsageWaitBlocks) : 0;
    YDC_LAUNCH(c, "k_usage_accrue", k_usage_accrue, dim3(l_blocks + w_blocks), dim3(256), 0, c->stream, sm.lt,
               sm.d_insp_rec.p, sm.d_insp_pre.p, l_blocks, with_w ? (rpc ? sm.rw.ip : sm.wq.ip) : nullptr,
               rpc ? sm.rw.n_imm : nullptr, rpc ? sm.rw.n_pre : nullptr, sm.ws, k.max_waiting, u.tb, u.z_dq, a.lh, u.z_done,
               c->opt_requestor_combine ? 1u : 0u);
  }
  // With aliveness: the heartbeats' expiries into E (servant_alive.h). Here for the reason the book's
  // pass is here: once per tick on every path.
  if (sm.alive.on && k.max_updates)
    YDC_LAUNCH(c, "k_alive_beat", k_alive_beat, dim3(ceil_div(k.max_updates, 256)), dim3(256), 0, c->stream, a.upd_idx,
               a.upd_exp, k.max_updates, std::min(S, sm.alive.n), sm.alive.col.p);
  YDC_LAUNCH(c, "k_lease_renew", k_lease_renew, dim3(std::max(1u, ceil_div(std::max(k.max_renewals, sm.lookback_n), 256))),
             dim3(256), 0, c->stream, sm.lt, sm.ls, in, k.max_renewals, sm.ren_slot, sm.z_renewed, sm.lookback,
             sm.lookback_n);
  if (k.max_renewals + k.max_frees)
    YDC_LAUNCH(c, "k_lease_free", k_lease_free, dim3(ren_blocks + ceil_div(k.max_frees, 256)), dim3(256), 0, c->stream,
               sm.lt, sm.ls, in, k.max_renewals, ren_blocks, sm.ren_slot, k.max_frees, S, c->d_running.p);
  // With departure: the staged requestors' leases freed, behind the caller's own frees and in front of
  // the reports and the sweep (stream_depart.h). Here for the reason the book's pass is here: once per
  // tick on every path.
  if (sm.max_depart) {
    const uint32_t MX = sm.max_depart;
    YDC_LAUNCH(c, "k_depart_load", k_depart_load, dim3(ceil_div(MX, 256)), dim3(256), 0, c->stream, a.dp_ip, a.dp_n, MX,
               sm.depart.list);
    YDC_LAUNCH(c, "k_depart_leases", k_depart_leases, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream,
               sm.lt, sm.ls, sm.d_insp_rec.p, sm.depart.list, MX, S, c->d_running.p);
  }
  if (k.max_reports)
    YDC_LAUNCH(c, "k_lease_report", k_lease_report, dim3(rep_blocks + ceil_div(k.max_report_ids, 256)), dim3(256), 0,
               c->stream, sm.lt, sm.ls, in, k.max_reports, rep_blocks, k.max_report_ids, S, sm.d_rep_tick.p, sm.z_unknown);
  // With a running-task book: the reports' permitted ids replace their servants' entries. Here and
  // nowhere else: this part of the step runs once per tick on every path, and the eager exits
  // place it no second time.
  if (sm.max_book)
    YDC_LAUNCH(c, "k_book_commit", k_book_commit, dim3(ceil_div(sm.max_book + k.max_report_ids, kBookTile)), dim3(256),
               0, c->stream, sm.book.bk, sm.book.bks, sm.max_book, in, a.bk_stid, a.bk_dkey, k.max_reports, k.max_report_ids,
               S, sm.d_rep_tick.p, sm.z_unknown, sm.book.lb, sm.book.z_bout);
  YDC_LAUNCH(c, "k_lease_sweep", k_lease_sweep, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream,
             sm.lt, sm.ls, a.lh, S, sm.d_rep_tick.p, c->d_running.p);
}

// With inspection on: what the granting pass files beside a lease (stream_inspect.h). env / ip: the
// placed batch's columns as the pass indexes them.
InspectIn inspect_in(ydc_context* c, const uint32_t* env, const uint32_t* ip) {
  auto& sm = c->stream_mode;
  return InspectIn{sm.d_insp_rec.p, sm.d_insp_pre.p, sm.inspect.ever.p, std::min(sm.inspect.n, c->reg.n),
                   env,             ip,              sm.rp.n_imm,      sm.rpc() ? sm.caps.max_waiting + sm.caps.max_tasks : 0};
}

// ... and behind the batch: ids for the grants, their leases, the answers, the outcome block. prm:
// gated on the batch having become final (the captured step); NULL: the host has just placed it.
void enqueue_lease_grant(ydc_context* c, const TickArena& a, const DeviceParams* prm, uint32_t check_slot) {
  auto& sm = c->stream_mode;
  if (sm.inspect.on) {
    YDC_LAUNCH(c, "k_lease_grant_inspect", k_lease_grant_inspect, dim3(ceil_div(sm.caps.max_tasks, kLeaseTile)), dim3(256),
               0, c->stream, sm.lt_out, sm.caps.max_tasks, a.lexp, a.lh, sm.lt, sm.ls, sm.lookback, sm.z_out, sm.z_task_id,
               sm.z_lout, prm, check_slot, inspect_in(c, a.env, a.ip));
    return;
  }
  YDC_LAUNCH(c, "k_lease_grant", k_lease_grant, dim3(ceil_div(sm.caps.max_tasks, kLeaseTile)), dim3(256), 0, c->stream,
             sm.lt_out, sm.caps.max_tasks, a.lexp, a.lh, sm.lt, sm.ls, sm.lookback, sm.z_out, sm.z_task_id, sm.z_lout,
             prm, check_slot);
}

// Waiting and leased at once, behind the batch: the one pass of wait_lease.h instead of the two
// above. prm as there.
void enqueue_wait_lease_commit(ydc_context* c, const TickArena& a, const DeviceParams* prm, uint32_t check_slot) {
  auto& sm = c->stream_mode;
  const uint32_t N = stream_batch_n(sm);
  if (sm.inspect.on) {
    YDC_LAUNCH(c, "k_wait_lease_commit_inspect", k_wait_lease_commit_inspect, dim3(ceil_div(N, kWaitTile)), dim3(256),
               0, c->stream, sm.wt, sm.wl, sm.wt_out, a.lh, sm.caps.max_waiting, N, sm.wq, sm.ws, sm.lt, sm.ls, sm.lookback,
               sm.z_out, sm.z_task_id, sm.z_res_tag, sm.z_res_idx, sm.z_wout, sm.z_lout, prm, check_slot,
               inspect_in(c, sm.wt.env, sm.wt.ip));
    return;
  }
  YDC_LAUNCH(c, "k_wait_lease_commit", k_wait_lease_commit, dim3(ceil_div(N, kWaitTile)), dim3(256), 0, c->stream,
             sm.wt, sm.wl, sm.wt_out, a.lh, sm.caps.max_waiting, N, sm.wq, sm.ws, sm.lt, sm.ls, sm.lookback, sm.z_out,
             sm.z_task_id, sm.z_res_tag, sm.z_res_idx, sm.z_wout, sm.z_lout, prm, check_slot);
}

// RPC mode, behind the batch: ids and leases per granted row, then every RPC settled. prm as above.
void enqueue_rpc_answer(ydc_context* c, const TickArena& a, const DeviceParams* prm, uint32_t check_slot) {
  auto& sm = c->stream_mode;
  const uint32_t P = sm.caps.max_waiting + sm.caps.max_tasks, NR = sm.caps.max_rows;
  if (sm.inspect.on)
    YDC_LAUNCH(c, "k_rpc_grant_inspect", k_rpc_grant_inspect, dim3(ceil_div(NR, kRpcTile)), dim3(256), 0, c->stream,
               sm.rb, NR, sm.caps.max_waiting, a.lh, sm.lt, sm.ls, sm.rs, sm.lb_grant, sm.rz, prm, check_slot,
               inspect_in(c, sm.rb.env, sm.rb.ip));
  else
    YDC_LAUNCH(c, "k_rpc_grant", k_rpc_grant, dim3(ceil_div(NR, kRpcTile)), dim3(256), 0, c->stream, sm.rb, NR,
               sm.caps.max_waiting, a.lh, sm.lt, sm.ls, sm.rs, sm.lb_grant, sm.rz, prm, check_slot);
  YDC_LAUNCH(c, "k_rpc_settle", k_rpc_settle, dim3(ceil_div(P, kRpcTile)), dim3(256), 0, c->stream, sm.rp, sm.rb,
             sm.caps.max_waiting, P, NR, a.lh, sm.rw, sm.ws, sm.rs, sm.ls, sm.lb_settle, sm.rz, sm.z_lout, prm,
             check_slot);
}

// The kernel behind the batch that answers the caller in the context's mode (none: a plain one).
void enqueue_stream_answer(ydc_context* c, const TickArena& a, const DeviceParams* prm, uint32_t check_slot) {
  auto& sm = c->stream_mode;
  if (sm.rpc()) enqueue_rpc_answer(c, a, prm, check_slot);
  else if (sm.waiting() && sm.leased()) enqueue_wait_lease_commit(c, a, prm, check_slot);
  else if (sm.waiting()) enqueue_wait_compact(c, a.now, prm, check_slot);
  else if (sm.leased()) enqueue_lease_grant(c, a, prm, check_slot);
  // With withdrawal: the withdrawn entries' label in the resolved list the pass above wrote, and the
  // counts (stream_withdraw.h), under the same gate.
  if (sm.max_withdraw) {
    const bool rpc = sm.rpc();
    YDC_LAUNCH(c, "k_withdraw_label", k_withdraw_label, dim3(ceil_div(std::max(sm.caps.max_waiting, sm.max_withdraw), 256)),
               dim3(256), 0, c->stream, sm.withdraw.list, sm.max_withdraw, rpc ? sm.rz.res_tag : sm.z_res_tag,
               rpc ? sm.rz.res_status : sm.z_res_idx, rpc ? &sm.rz.outcome->n_resolved : &sm.z_wout->n_resolved,
               sm.caps.max_waiting, sm.withdraw.z_count, sm.withdraw.z_done, prm, check_slot);
  }
  // With departure: the counts to the page-locked result block, under the same gate (stream_depart.h).
  if (sm.max_depart)
    YDC_LAUNCH(c, "k_depart_done", k_depart_done, dim3(ceil_div(sm.max_depart, 256)), dim3(256), 0, c->stream,
               sm.depart.list, sm.max_depart, a.lh, sm.depart.z_count, sm.depart.z_done, prm, check_slot);
  // With a quota: the table cleared for the next tick, and under the commit pass's gate the label of the
  // requests that were admitted nothing, the admitted counts and the result block (stream_quota.h).
  if (sm.quota.on) {
    const auto& q = sm.quota;
    const bool rpc = sm.rpc();
    YDC_LAUNCH(c, "k_quota_label", k_quota_label, dim3(ceil_div(std::max(sm.caps.max_tasks, q.tb.mask + 1), 256)),
               dim3(256), 0, c->stream, q.tb, q.tk, a.q_n, sm.caps.max_tasks, a.lh, rpc ? sm.rz.status : sm.z_out, q.z_imm,
               rpc ? q.z_pre : nullptr, q.z_done, prm, check_slot);
    // With the fair-share level: its result block, under the same gate (stream_fair.h).
    if (q.fair_on())
      YDC_LAUNCH(c, "k_fair_done", k_fair_done, dim3(1), dim3(64), 0, c->stream, q.fair.res, q.z_fres, prm, check_slot);
  }
}

// The step itself, enqueued on the context's stream (inside a capture, or — stream_graph=0 — as it is).
int stream_enqueue_step(ydc_context* c, const BatchPlan& plan, bool by_swap) {
  auto& sm = c->stream_mode;
  hipStream_t st = c->stream;
  int rc = YDC_OK;
  auto cap = [&](hipError_t e) {
    if (e != hipSuccess && rc == YDC_OK)
      rc = fail(c, YDC_ERR_HIP, "streaming step: %s", hipGetErrorString(e));
  };
  // No copy node. The tick's inputs are read where the host put them (k_apply_tick and the request
  // classification read every word once), the placement is stored to the page-locked result array
  // by k_finalize, and so is the outcome block (outcome_store=0: copied).
  // Leased mode: the lease kernels of the tick's renewals, frees, reports and expiry come first
  // (their decrements of running_tasks and k_apply_tick's commute); the placement stays in HBM
  // for k_lease_grant, which answers the caller.
  const bool leased = sm.leased();
  if (leased) enqueue_lease_pre(c, sm.z);
  enqueue_apply_tick(c, sm.z);
  // Waiting mode: the batch is W's region and the new requests, gathered into HBM; its placement
  // stays there for k_wait_compact, which answers the caller.
  const bool waiting = sm.waiting();
  if (waiting) enqueue_stream_gather(c, sm.z);
  ydc_task_soa d{sm.z.env, sm.z.minv, sm.z.ip};
  if (waiting) d = ydc_task_soa{sm.wt.env, sm.wt.minv, sm.wt.ip};
  // (the captured step decides the finalise for itself: by_swap is the capture's, the outcome block the context's)
  const bool outcome_stored = c->opt_outcome_store && plan.S != 0;
  BatchCall call;
  call.flags = YDC_DISPATCH_COMMIT;
  call.out_idx = waiting ? sm.wt_out : leased ? sm.lt_out : sm.z_out;
  call.outcome = outcome_stored ? c->h_prm.dev() : nullptr;
  call.by_swap = by_swap;
  if (rc == YDC_OK) rc = enqueue_front(c, plan, &d, call);
  if (rc == YDC_OK && plan.wave_path)
    for (uint32_t r = 0; r < sm.passes; ++r) enqueue_pass(c, plan, r, 1u);
  const uint32_t check_slot = plan.wave_path ? (sm.passes - 1) & 63 : kNone;
  if (rc == YDC_OK) rc = enqueue_finalize(c, plan, call, check_slot);
  if (rc == YDC_OK) enqueue_stream_answer(c, sm.z, c->d_prm.p, check_slot);
  if (!outcome_stored) cap(hipMemcpyAsync(c->h_prm, c->d_prm.p, sizeof(DeviceParams), hipMemcpyDeviceToHost, st));
  return rc;
}

// One capture of the step with the columns as they are now (plan: made for them).
int stream_capture_one(ydc_context* c, const BatchPlan& plan, bool by_swap, hipGraph_t* g_out,
                       hipGraphExec_t* e_out) {
  hipStream_t st = c->stream;
  HIP_TRY(c, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  const int rc = stream_enqueue_step(c, plan, by_swap);
  hipGraph_t g = nullptr;
  hipError_t ee = hipStreamEndCapture(st, &g);
  if (ee != hipSuccess) return fail(c, YDC_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ee));
  if (rc != YDC_OK) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  *g_out = g;
  HIP_TRY(c, hipGraphInstantiate(e_out, g, nullptr, nullptr, 0));
  return YDC_OK;
}

int stream_capture(ydc_context* c) {
  auto& sm = c->stream_mode;
  stream_drop_graphs(sm);
  const bool was_profiling = c->profiling;
  c->profiling = false;  // no event pairs inside a capture
  // Sizes and workspace first (allocations and table uploads cannot be captured).
  if (sm.leased() && sm.d_rep_tick.cap < c->reg.n) {
    // (a tick number is never 0, and a servant's stamp matters within its tick only)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, sm.d_rep_tick.reserve((size_t)c->reg.n + 1024));
    HIP_TRY(c, hipMemset(sm.d_rep_tick.p, 0, sm.d_rep_tick.cap * 4));
  }
  if (int rc = plan_batch(c, stream_batch_n(sm), &sm.plan)) return rc;
  if (sm.plan.use_generic) {
    // More than 256 servant classes: the rounds of that path are checked by the host, which a
    // captured step cannot do — such ticks run eagerly (ydc_stream_tick_wide, below).
    c->profiling = was_profiling;
    sm.eager_only = true;
    sm.stale = false;
    return YDC_OK;
  }
  sm.eager_only = false;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  sm.passes = sm.want_passes ? sm.want_passes : std::max(2u, std::min(c->round_hint + 1, 12u));
  sm.window_max = sm.window_ticks = 0;
  sm.swaps = c->opt_commit_swap && sm.plan.S != 0;
  sm.run_a = c->d_running.p;
  int rc = stream_capture_one(c, sm.plan, sm.swaps, &sm.graph, &sm.exec);
  if (rc == YDC_OK && sm.swaps) {
    // ... and once more with the two columns in each other's role.
    std::swap(c->d_running, c->d_running_out);
    sm.run_b = c->d_running.p;
    rc = plan_batch(c, stream_batch_n(sm), &sm.plan_b);
    if (rc == YDC_OK) rc = stream_capture_one(c, sm.plan_b, true, &sm.graph_b, &sm.exec_b);
    std::swap(c->d_running, c->d_running_out);
  }
  c->profiling = was_profiling;
  if (rc != YDC_OK) return rc;
  sm.stale = false;
  return YDC_OK;
}

// A waiting tick's own arguments (ydc_stream_tick_waiting).
struct WaitTick {
  const int64_t* deadlines;
  const uint64_t* tags;
  int64_t now;
  uint64_t* out_resolved_tags;
  uint32_t* out_resolved_idx;
  uint32_t* out_n_resolved;
  uint32_t* out_n_waiting;
  uint64_t* out_resolved_task_id;  // waiting and leased at once; NULL otherwise
};

// A leased tick's own arguments (ydc_stream_tick_leased).
struct LeaseTick {
  const uint64_t* renew_id;
  const int64_t* renew_exp;
  uint32_t n_renew;
  const uint64_t* free_id;
  uint32_t n_free;
  const uint32_t *rep_srv, *rep_off;
  const uint64_t* rep_id;
  uint32_t n_rep;
  const int64_t* lease_exp;
  int64_t now;
  uint64_t* out_task_id;
  uint8_t *out_renewed, *out_unknown;
  uint32_t* out_n_leases;
};

// An rpc tick's own arguments (ydc_stream_tick_rpc), beside a waiting and a leased tick's.
struct RpcTick {
  const uint32_t *n_imm, *n_pre;
  uint32_t *out_status, *out_n_granted;
  uint32_t *out_resolved_n_granted, *out_resolved_first, *out_resolved_servant_idx;
  uint32_t* out_n_waiting_rows;
};

// What a tick brings, whichever entry point took it: the heartbeats (with their environment masks
// in the wide form), the releases, the requests, where the placement goes, and the mode's own
// arguments (NULL: not a tick of that mode).
struct StreamCall {
  const uint32_t* upd_idx;
  const ydc_servant_row* upd_rows;
  const uint64_t* upd_env_masks;
  uint32_t env_words, n_upd;
  const uint32_t* rel;
  uint32_t n_rel;
  const ydc_task_soa* tasks;
  uint32_t n_tasks;
  uint32_t* out_servant_idx;
  const WaitTick* wt;
  const LeaseTick* lt;
  const RpcTick* rt;
};

// The limits of a stream's bounds; `code`: what going beyond them is to the caller.
int stream_caps_check(ydc_context* c, int code, const ydc_stream_caps& k, uint32_t max_book) {
  // (the book's pass is over max_book + max_report_ids positions, one 31-bit count)
  if (max_book && (!k.max_leases || max_book > (1u << 30) || (uint64_t)max_book + k.max_report_ids > 0x7FFFFFFFull))
    return fail(c, code, "max_book %u out of range (1 .. 2^30, max_book + max_report_ids < 2^31)", max_book);
  // (rpc mode: max_tasks is max_requests, the batch is the max_rows expanded rows)
  if (k.max_rows && (k.max_rows > (1u << 30) || k.max_rows < k.max_tasks))
    return fail(c, code, "max_rows %u out of range (max_requests %u .. 2^30)", k.max_rows, k.max_tasks);
  if (k.max_leases && (k.max_leases > (1u << 30) || k.max_report_ids > 0x7FFFFFFFu))
    return fail(c, code, "max_leases %u out of range (1 .. 2^30)", k.max_leases);
  if ((uint64_t)k.max_tasks + k.max_waiting > 0x7FFFFFFFull)
    return fail(c, code, "max_tasks %u + max_waiting %u too large", k.max_tasks, k.max_waiting);
  return YDC_OK;
}

// The record's bounds, listed once, in the order the snapshot codec numbers them (snap::Cap).
constexpr uint32_t ydc_stream_caps::*kCapFields[snap::kCaps] = {
    &ydc_stream_caps::max_updates, &ydc_stream_caps::max_releases, &ydc_stream_caps::max_tasks,
    &ydc_stream_caps::max_rows,    &ydc_stream_caps::max_waiting,  &ydc_stream_caps::max_leases,
    &ydc_stream_caps::max_renewals, &ydc_stream_caps::max_frees,   &ydc_stream_caps::max_reports,
    &ydc_stream_caps::max_report_ids};

// `have` grown to what `want` asks for: no bound shrinks.
ydc_stream_caps stream_caps_grown(const ydc_stream_caps& have, const ydc_stream_caps& want) {
  ydc_stream_caps k{};
  for (auto f : kCapFields) k.*f = std::max(have.*f, want.*f);
  return k;
}

// The mode of a stream is fixed: what `want` asks of a part that a stream with the bounds `have`
// was begun without, or NULL.
const char* stream_caps_foreign(const ydc_stream_caps& have, const ydc_stream_caps& want) {
  if (!have.max_waiting && want.max_waiting) return "max_waiting for a stream without a waiting queue";
  if (!have.max_leases &&
      (want.max_leases | want.max_renewals | want.max_frees | want.max_reports | want.max_report_ids))
    return "lease capacities for a stream without a lease table";
  if (!have.max_rows && want.max_rows) return "max_rows for a stream that is not an rpc stream";
  return nullptr;
}

// Layout and allocation of everything a stream of these bounds has, into `sm` (released, or
// fresh). Its contents are not defined before stream_reset; after a failure the caller releases it.
int stream_alloc(ydc_context* c, ydc_context::Stream& sm, const ydc_stream_caps& k, uint32_t max_book,
                 uint32_t max_withdraw, uint32_t quota, uint32_t max_depart) {
  sm.caps = k;
  sm.max_book = max_book;
  sm.max_withdraw = max_withdraw;
  sm.max_depart = max_depart;
  sm.quota.on = quota != 0;  // (Stream::Quota::code)
  sm.quota.max_overrides = quota ? quota - 1 : 0;
  const uint32_t max_updates = k.max_updates, max_releases = k.max_releases, max_tasks = k.max_tasks;
  const uint32_t max_waiting = k.max_waiting, max_rows = k.max_rows;
  const bool leased = sm.leased();
  // Arena layout (256 B aligned sections); waiting mode adds the new requests' deadlines and tags,
  // and the tick's clock.
  size_t off = 0;
  const size_t o_idx = section(&off, (size_t)max_updates * 4);
  const size_t o_rows = section(&off, (size_t)max_updates * sizeof(ydc_servant_row));
  const size_t o_rel = section(&off, (size_t)max_releases * 4);
  const size_t o_env = section(&off, (size_t)max_tasks * 4);
  const size_t o_minv = section(&off, (size_t)max_tasks * 4);
  const size_t o_ip = section(&off, (size_t)max_tasks * 4);
  const size_t o_dl = max_waiting ? section(&off, (size_t)max_tasks * 8) : 0;
  const size_t o_tag = max_waiting ? section(&off, (size_t)max_tasks * 8) : 0;
  const size_t o_now = max_waiting ? section(&off, 8) : 0;
  // ... leased mode the requests' expiries, renewals, frees by id, reports (CSR) and the scalars.
  const size_t o_lexp = leased ? section(&off, (size_t)max_tasks * 8) : 0;
  const size_t o_ren_id = leased ? section(&off, (size_t)k.max_renewals * 8) : 0;
  const size_t o_ren_exp = leased ? section(&off, (size_t)k.max_renewals * 8) : 0;
  const size_t o_free_id = leased ? section(&off, (size_t)k.max_frees * 8) : 0;
  const size_t o_rep_srv = leased ? section(&off, (size_t)k.max_reports * 4) : 0;
  const size_t o_rep_off = leased ? section(&off, ((size_t)k.max_reports + 1) * 4) : 0;
  const size_t o_rep_id = leased ? section(&off, (size_t)k.max_report_ids * 8) : 0;
  const size_t o_lh = leased ? section(&off, sizeof(LeaseHdr)) : 0;
  const size_t o_nimm = max_rows ? section(&off, (size_t)max_tasks * 4) : 0;
  const size_t o_npre = max_rows ? section(&off, (size_t)max_tasks * 4) : 0;
  // ... a running-task book the reports' two payload columns.
  const size_t o_bstid = max_book ? section(&off, (size_t)k.max_report_ids * 8) : 0;
  const size_t o_bdkey = max_book ? section(&off, (size_t)k.max_report_ids * 8) : 0;
  // ... and, last (no other section moves), the heartbeats' expiries of a leased stream.
  const size_t o_uexp = leased ? section(&off, (size_t)max_updates * 8) : 0;
  // ... and behind it, with withdrawal, the staged tags and their number.
  const size_t o_wdt = max_withdraw ? section(&off, (size_t)max_withdraw * 8) : 0;
  const size_t o_wdn = max_withdraw ? section(&off, 4) : 0;
  // ... and behind that, with a quota, the number of the tick's new requests.
  const size_t o_qn = quota ? section(&off, 4) : 0;
  // ... and last, with departure, the staged requestors and their number.
  const size_t o_dpi = max_depart ? section(&off, (size_t)max_depart * 4) : 0;
  const size_t o_dpn = max_depart ? section(&off, 4) : 0;
  auto arena_at = [&](uint8_t* b) {
    TickArena a{(uint32_t*)(b + o_idx), (ydc_servant_row*)(b + o_rows), (uint32_t*)(b + o_rel),
                (uint32_t*)(b + o_env), (uint32_t*)(b + o_minv), (uint32_t*)(b + o_ip),
                max_waiting ? (int64_t*)(b + o_dl) : nullptr, max_waiting ? (uint64_t*)(b + o_tag) : nullptr,
                max_waiting ? (int64_t*)(b + o_now) : nullptr};
    if (leased) {
      a.lexp = (int64_t*)(b + o_lexp);
      a.ren_id = (unsigned long long*)(b + o_ren_id);
      a.ren_exp = (int64_t*)(b + o_ren_exp);
      a.free_id = (unsigned long long*)(b + o_free_id);
      a.rep_srv = (uint32_t*)(b + o_rep_srv);
      a.rep_off = (uint32_t*)(b + o_rep_off);
      a.rep_id = (unsigned long long*)(b + o_rep_id);
      a.lh = (LeaseHdr*)(b + o_lh);
      a.upd_exp = (int64_t*)(b + o_uexp);
    }
    if (max_rows) {
      a.nimm = (uint32_t*)(b + o_nimm);
      a.npre = (uint32_t*)(b + o_npre);
    }
    if (max_book) {
      a.bk_stid = (unsigned long long*)(b + o_bstid);
      a.bk_dkey = (unsigned long long*)(b + o_bdkey);
    }
    if (max_withdraw) {
      a.wd_tag = (uint64_t*)(b + o_wdt);
      a.wd_n = (uint32_t*)(b + o_wdn);
    }
    if (quota) a.q_n = (uint32_t*)(b + o_qn);
    if (max_depart) {
      a.dp_ip = (uint32_t*)(b + o_dpi);
      a.dp_n = (uint32_t*)(b + o_dpn);
    }
    return a;
  };
  sm.in_bytes = off;
  HIP_TRY(c, sm.h_in.reserve(sm.in_bytes));
  const size_t n_out = max_rows ? max_rows : max_tasks;  // answers per tick (rpc mode: one per row)
  HIP_TRY(c, sm.h_place.reserve(n_out * 4));
  sm.h_out = (uint32_t*)sm.h_place.p;
  sm.z_out = (uint32_t*)sm.h_place.z;
  HIP_TRY(c, sm.d_in.reserve(sm.in_bytes));
  sm.h = arena_at(sm.h_in.p);
  sm.d = arena_at(sm.d_in.p);
  sm.z = arena_at(sm.h_in.z);
  HIP_TRY(c, c->d_out_idx.reserve(max_tasks));
  if (max_waiting) {
    // HBM: W (max_waiting entries), the tick's batch (max_waiting + max_tasks) with its placement,
    // the queue's counters and k_wait_compact's look-back words.
    const size_t NB = max_rows ? (size_t)max_rows : (size_t)max_tasks + max_waiting;
    sm.lookback_n = (uint32_t)((NB + kWaitTile - 1) / kWaitTile);
    size_t w_off = 0;
    auto wsec = [&](size_t bytes) { return section(&w_off, bytes); };
    const size_t o_wq[5] = {wsec(max_waiting * 4ull), wsec(max_waiting * 4ull), wsec(max_waiting * 4ull),
                            wsec(max_waiting * 8ull), wsec(max_waiting * 8ull)};
    const size_t o_wt[5] = {wsec(NB * 4), wsec(NB * 4), wsec(NB * 4), wsec(NB * 8), wsec(NB * 8)};
    const size_t o_wout = wsec(NB * 4), o_ws = wsec(sizeof(WaitState)), o_lb = wsec((size_t)sm.lookback_n * 8);
    // ... with leases: W's sixth column and the batch's, the lease durations (wait_lease.h).
    const size_t o_wfor = leased ? wsec(max_waiting * 8ull) : 0, o_tfor = leased ? wsec(NB * 8) : 0;
    HIP_TRY(c, sm.d_wait.reserve(w_off));
    uint8_t* b = sm.d_wait.p;
    if (leased) sm.wl = WaitLeaseCols{(int64_t*)(b + o_wfor), (int64_t*)(b + o_tfor), nullptr};
    sm.wq = WaitCols{(uint32_t*)(b + o_wq[0]), (uint32_t*)(b + o_wq[1]), (uint32_t*)(b + o_wq[2]),
                     (int64_t*)(b + o_wq[3]), (uint64_t*)(b + o_wq[4])};
    sm.wt = WaitCols{(uint32_t*)(b + o_wt[0]), (uint32_t*)(b + o_wt[1]), (uint32_t*)(b + o_wt[2]),
                     (int64_t*)(b + o_wt[3]), (uint64_t*)(b + o_wt[4])};
    sm.wt_out = (uint32_t*)(b + o_wout);
    sm.ws = (WaitState*)(b + o_ws);
    sm.lookback = (unsigned long long*)(b + o_lb);
    // Page-locked results: resolved tags | resolved answers | outcome block.
    size_t r_off = 0;
    const size_t r_tag = section(&r_off, (size_t)max_waiting * 8), r_idx = section(&r_off, (size_t)max_waiting * 4);
    const size_t r_out = section(&r_off, sizeof(WaitOutcome));
    const size_t r_id = leased ? section(&r_off, (size_t)max_waiting * 8) : 0;  // (with leases: the resolved ids)
    HIP_TRY(c, sm.h_wres.reserve(r_off));
    uint8_t *h_res = sm.h_wres.p, *z_res = sm.h_wres.z;
    if (leased) {
      sm.h_res_id = (unsigned long long*)(h_res + r_id);
      sm.wl.res_id = (unsigned long long*)(z_res + r_id);
    }
    sm.h_res_tag = (uint64_t*)(h_res + r_tag);
    sm.h_res_idx = (uint32_t*)(h_res + r_idx);
    sm.h_wout = (WaitOutcome*)(h_res + r_out);
    sm.z_res_tag = (uint64_t*)(z_res + r_tag);
    sm.z_res_idx = (uint32_t*)(z_res + r_idx);
    sm.z_wout = (WaitOutcome*)(z_res + r_out);
  }
  if (leased) {
    // HBM: the table (cap = 2^k >= 2 * max_leases slots, five columns), its bookkeeping, the
    // renewals' slots, the placement of the tick's batch and k_lease_grant's look-back words.
    size_t cap = 1024;
    uint32_t cap_bits = 10;
    while (cap < 2 * (size_t)k.max_leases) cap <<= 1, ++cap_bits;
    // (with a waiting queue: two words per tile of the whole batch, wait_lease.h)
    sm.lookback_n = max_waiting ? 2 * ceil_div(max_tasks + max_waiting, kWaitTile) : ceil_div(max_tasks, kLeaseTile);
    // (rpc mode: the scan's and the settling's words per tile of positions, the grants' per tile of rows)
    if (max_rows) sm.lookback_n = 2 * ceil_div(max_tasks + max_waiting, kRpcTile) + ceil_div(max_rows, kRpcTile);
    // (a running-task book: one word per tile of its pass, behind the others; k_lease_renew clears them all)
    const uint32_t lb_own = sm.lookback_n;
    if (max_book) sm.lookback_n += ceil_div(max_book + k.max_report_ids, kBookTile);
    size_t l_off = 0;
    auto lsec = [&](size_t bytes) { return section(&l_off, bytes); };
    const size_t o_key = lsec(cap * 8), o_exp = lsec(cap * 8), o_srv = lsec(cap * 4), o_st = lsec(cap * 4);
    const size_t o_win = lsec(cap * 4), o_ls = lsec(sizeof(LeaseState)), o_rs = lsec((size_t)k.max_renewals * 4);
    const size_t o_out = lsec((size_t)max_tasks * 4), o_lb = lsec((size_t)sm.lookback_n * 8);
    HIP_TRY(c, sm.d_lease.reserve(l_off));
    uint8_t* b = sm.d_lease.p;
    sm.lt = LeaseCols{(unsigned long long*)(b + o_key), (int64_t*)(b + o_exp), (uint32_t*)(b + o_srv),
                      (uint32_t*)(b + o_st), (uint32_t*)(b + o_win), (uint32_t)(cap - 1), 64 - cap_bits};
    sm.ls = (LeaseState*)(b + o_ls);
    sm.ren_slot = (uint32_t*)(b + o_rs);
    sm.lt_out = (uint32_t*)(b + o_out);
    sm.lookback = (unsigned long long*)(b + o_lb);
    sm.book.lb = max_book ? sm.lookback + lb_own : nullptr;
    // Page-locked results: task ids | renewed | report_unknown | outcome block.
    size_t r_off = 0;
    const size_t r_id = section(&r_off, n_out * 8), r_ren = section(&r_off, k.max_renewals);
    const size_t r_unk = section(&r_off, k.max_report_ids), r_out = section(&r_off, sizeof(LeaseOutcome));
    HIP_TRY(c, sm.h_lres.reserve(r_off));
    uint8_t *h_res = sm.h_lres.p, *z_res = sm.h_lres.z;
    sm.h_task_id = (unsigned long long*)(h_res + r_id);
    sm.h_renewed = h_res + r_ren;
    sm.h_unknown = h_res + r_unk;
    sm.h_lout = (LeaseOutcome*)(h_res + r_out);
    sm.z_task_id = (unsigned long long*)(z_res + r_id);
    sm.z_renewed = z_res + r_ren;
    sm.z_unknown = z_res + r_unk;
    sm.z_lout = (LeaseOutcome*)(z_res + r_out);
  }
  if (max_rows) {
    const size_t MW = max_waiting, P = MW + max_tasks, NR = max_rows;
    const uint32_t tiles_p = ceil_div((uint32_t)P, kRpcTile);
    sm.lb_scan = sm.lookback;
    sm.lb_settle = sm.lookback + tiles_p;
    sm.lb_grant = sm.lookback + 2 * (size_t)tiles_p;
    // HBM: W's two count columns, the positions' eight columns, row_start, rank, the tickets.
    size_t d_off = 0;
    auto dsec = [&](size_t bytes) { return section(&d_off, bytes); };
    const size_t o_wi = dsec(MW * 4), o_wp = dsec(MW * 4);
    const size_t o_p4[5] = {dsec(P * 4), dsec(P * 4), dsec(P * 4), dsec(P * 4), dsec(P * 4)};
    const size_t o_p8[3] = {dsec(P * 8), dsec(P * 8), dsec(P * 8)};
    const size_t o_rs = dsec((P + 1) * 4), o_rk = dsec((NR + 1) * 4), o_st = dsec(sizeof(RpcState));
    HIP_TRY(c, sm.d_rpc.reserve(d_off));
    uint8_t* b = sm.d_rpc.p;
    sm.rw = RpcEntryCols{sm.wq.env, sm.wq.minv, sm.wq.ip, sm.wq.deadline, sm.wq.tag, sm.wl.w_for,
                         (uint32_t*)(b + o_wi), (uint32_t*)(b + o_wp)};
    sm.rp = RpcEntryCols{(uint32_t*)(b + o_p4[0]), (uint32_t*)(b + o_p4[1]), (uint32_t*)(b + o_p4[2]),
                         (int64_t*)(b + o_p8[0]), (uint64_t*)(b + o_p8[1]), (int64_t*)(b + o_p8[2]),
                         (uint32_t*)(b + o_p4[3]), (uint32_t*)(b + o_p4[4])};
    sm.rb = RpcBatch{sm.wt.env, sm.wt.minv, sm.wt.ip, sm.wl.t_for, sm.wt_out, (uint32_t*)(b + o_rk),
                     (uint32_t*)(b + o_rs)};
    sm.rs = (RpcState*)(b + o_st);
    // Page-locked results beside h_out / h_task_id (the new requests' rows): status and count per
    // request, the resolved list, W's grants packed, the outcome block.
    size_t r_off = 0;
    auto rsec = [&](size_t bytes) { return section(&r_off, bytes); };
    const size_t r_st = rsec((size_t)max_tasks * 4), r_ng = rsec((size_t)max_tasks * 4);
    const size_t r_tag = rsec(MW * 8), r_rs = rsec(MW * 4), r_rn = rsec(MW * 4), r_rf = rsec(MW * 4);
    const size_t r_srv = rsec(NR * 4), r_id = rsec(NR * 8), r_out = rsec(sizeof(RpcOutcome));
    HIP_TRY(c, sm.h_rres.reserve(r_off));
    auto out_at = [&](uint8_t* q, uint32_t* srv, unsigned long long* id) {
      return RpcOut{srv, id, (uint32_t*)(q + r_st), (uint32_t*)(q + r_ng), (uint64_t*)(q + r_tag),
                    (uint32_t*)(q + r_rs), (uint32_t*)(q + r_rn), (uint32_t*)(q + r_rf), (uint32_t*)(q + r_srv),
                    (unsigned long long*)(q + r_id), (RpcOutcome*)(q + r_out)};
    };
    sm.rh = out_at(sm.h_rres.p, sm.h_out, sm.h_task_id);
    sm.rz = out_at(sm.h_rres.z, sm.z_out, sm.z_task_id);
  }
  if (max_book) {
    // HBM: B's four columns and its bookkeeping. Page-locked: the outcome block.
    size_t b_off = 0;
    auto bsec = [&](size_t bytes) { return section(&b_off, bytes); };
    const size_t o_srv = bsec((size_t)max_book * 4), o_gr = bsec((size_t)max_book * 8);
    const size_t o_st = bsec((size_t)max_book * 8), o_dk = bsec((size_t)max_book * 8), o_bs = bsec(sizeof(BookState));
    HIP_TRY(c, sm.book.d.reserve(b_off));
    uint8_t* b = sm.book.d.p;
    sm.book.bk = BookCols{(uint32_t*)(b + o_srv), (unsigned long long*)(b + o_gr), (unsigned long long*)(b + o_st),
                     (unsigned long long*)(b + o_dk)};
    sm.book.bks = (BookState*)(b + o_bs);
    HIP_TRY(c, sm.book.h_res.reserve(256));
    sm.book.h_bout = (BookOutcome*)sm.book.h_res.p;
    sm.book.z_bout = (BookOutcome*)sm.book.h_res.z;
  }
  if (max_withdraw) {
    // HBM: the tick's list, its counts and its length. Page-locked: the counts and the done block.
    size_t d_off = 0, r_off = 0;
    const size_t o_tag = section(&d_off, (size_t)max_withdraw * 8), o_cnt = section(&d_off, (size_t)max_withdraw * 4);
    const size_t o_n = section(&d_off, 4);
    HIP_TRY(c, sm.withdraw.d.reserve(d_off));
    uint8_t* b = sm.withdraw.d.p;
    sm.withdraw.list = WithdrawList{(unsigned long long*)(b + o_tag), (uint32_t*)(b + o_cnt), (uint32_t*)(b + o_n)};
    const size_t r_cnt = section(&r_off, (size_t)max_withdraw * 4), r_done = section(&r_off, sizeof(WithdrawDone));
    HIP_TRY(c, sm.withdraw.h_res.reserve(r_off));
    sm.withdraw.h_count = (uint32_t*)(sm.withdraw.h_res.p + r_cnt);
    sm.withdraw.z_count = (uint32_t*)(sm.withdraw.h_res.z + r_cnt);
    sm.withdraw.h_done = (WithdrawDone*)(sm.withdraw.h_res.p + r_done);
    sm.withdraw.z_done = (WithdrawDone*)(sm.withdraw.h_res.z + r_done);
  }
  if (max_depart) {
    // HBM: the tick's list, its counts and its length. Page-locked: the counts and the done block.
    auto& dp = sm.depart;
    size_t d_off = 0, r_off = 0;
    const size_t o_ip = section(&d_off, (size_t)max_depart * 4), o_cnt = section(&d_off, (size_t)max_depart * 16);
    const size_t o_n = section(&d_off, 4);
    HIP_TRY(c, dp.d.reserve(d_off));
    uint8_t* b = dp.d.p;
    dp.list = DepartList{(uint32_t*)(b + o_ip), (uint4*)(b + o_cnt), (uint32_t*)(b + o_n)};
    const size_t r_cnt = section(&r_off, (size_t)max_depart * 16), r_done = section(&r_off, sizeof(DepartDone));
    HIP_TRY(c, dp.h_res.reserve(r_off));
    dp.h_count = (uint4*)(dp.h_res.p + r_cnt);
    dp.z_count = (uint4*)(dp.h_res.z + r_cnt);
    dp.h_done = (DepartDone*)(dp.h_res.p + r_done);
    dp.z_done = (DepartDone*)(dp.h_res.z + r_done);
  }
  if (quota) {
    // HBM: the table (word | held | asked), the settings, the per-request arrays, the counters and the
    // chain words. Page-locked: the admitted counts and the done block.
    auto& q = sm.quota;
    const uint32_t slots = quota_slots(max_tasks), MO = q.max_overrides;
    q.tiles = ceil_div(max_tasks, kQuotaTile);
    size_t d_off = 0, r_off = 0;
    auto qsec = [&](size_t bytes) { return section(&d_off, bytes); };
    const size_t o_word = qsec((size_t)slots * 8), o_held = qsec((size_t)slots * 4), o_asked = qsec((size_t)slots * 4);
    const size_t o_oip = qsec((size_t)MO * 4), o_ocap = qsec((size_t)MO * 4), o_hdr = qsec(8);
    const size_t o_slot = qsec((size_t)max_tasks * 4), o_imm = qsec((size_t)max_tasks * 4);
    const size_t o_pre = qsec((size_t)max_tasks * 4), o_env = qsec((size_t)max_tasks * 4);
    const size_t o_cnt = qsec(16), o_chain = qsec((size_t)q.tiles * 4);
    HIP_TRY(c, q.d.reserve(d_off));
    uint8_t* b = q.d.p;
    q.tb = QuotaTable{(unsigned long long*)(b + o_word), (uint32_t*)(b + o_held), (uint32_t*)(b + o_asked), slots - 1};
    q.caps = QuotaCaps{(uint32_t*)(b + o_oip), (uint32_t*)(b + o_ocap), (uint32_t*)(b + o_hdr), MO};
    q.tk = QuotaTick{(uint32_t*)(b + o_slot), (uint32_t*)(b + o_imm), (uint32_t*)(b + o_pre), (uint32_t*)(b + o_env),
                     (uint32_t*)(b + o_cnt), (uint32_t*)(b + o_chain)};
    const size_t r_imm = section(&r_off, (size_t)max_tasks * 4), r_pre = section(&r_off, (size_t)max_tasks * 4);
    const size_t r_done = section(&r_off, sizeof(QuotaDone));
    HIP_TRY(c, q.h_res.reserve(r_off));
    q.h_imm = (uint32_t*)(q.h_res.p + r_imm);
    q.z_imm = (uint32_t*)(q.h_res.z + r_imm);
    q.h_pre = (uint32_t*)(q.h_res.p + r_pre);
    q.z_pre = (uint32_t*)(q.h_res.z + r_pre);
    q.h_done = (QuotaDone*)(q.h_res.p + r_done);
    q.z_done = (QuotaDone*)(q.h_res.z + r_done);
    // The fair-share level's columns (stream_fair.h): ask | the list of pairs | sums |
    // the tick's header | the result | the settings.
    size_t f_off = 0;
    const size_t f_ask = section(&f_off, (size_t)slots * 4);
    const size_t f_pair = section(&f_off, (size_t)slots * 8);
    const size_t f_sums = section(&f_off, sizeof(FairSums)), f_hdr = section(&f_off, 8);
    const size_t f_res = section(&f_off, sizeof(FairResult)), f_set = section(&f_off, sizeof(FairSet));
    HIP_TRY(c, q.fd.reserve(f_off));
    uint8_t* fb = q.fd.p;
    q.fair = FairTick{(uint32_t*)(fb + f_ask), (uint2*)(fb + f_pair), (FairSums*)(fb + f_sums), (uint32_t*)(fb + f_hdr),
                      (FairResult*)(fb + f_res), (const FairSet*)(fb + f_set)};
    HIP_TRY(c, q.h_fair.reserve(sizeof(FairResult)));
    q.h_fres = (FairResult*)q.h_fair.p;
    q.z_fres = (FairResult*)q.h_fair.z;
  }
  sm.want_passes = sm.window_max = sm.window_ticks = 0;
  sm.stale = true;
  return YDC_OK;
}

// The state of a stream that has just been begun, in the buffers stream_alloc made: W empty, L
// empty with next_id 0 (the reference's next_task_id{}), the rpc columns and every outcome block
// cleared.
int stream_reset(ydc_context* c, ydc_context::Stream& sm) {
  if (sm.waiting()) {
    HIP_TRY(c, hipMemsetAsync(sm.ws, 0, sizeof(WaitState), c->stream));
    std::memset(sm.h_wout, 0, sizeof(WaitOutcome));
  }
  if (sm.leased()) {
    HIP_TRY(c, hipMemsetAsync(sm.d_lease.p, 0, sm.d_lease.cap, c->stream));
    HIP_TRY(c, hipMemsetAsync(sm.lt.key, 0xFF, ((size_t)sm.lt.mask + 1) * 8, c->stream));
    std::memset(sm.h_lout, 0, sizeof(LeaseOutcome));
  }
  if (sm.rpc()) {
    HIP_TRY(c, hipMemsetAsync(sm.d_rpc.p, 0, sm.d_rpc.cap, c->stream));
    std::memset(sm.rh.outcome, 0, sizeof(RpcOutcome));
  }
  if (sm.max_book) {  // (B empty, the ticket 0)
    HIP_TRY(c, hipMemsetAsync(sm.book.bks, 0, sizeof(BookState), c->stream));
    std::memset(sm.book.h_bout, 0, sizeof(BookOutcome));
    sm.book.n = 0;
  }
  if (sm.max_withdraw) {  // (an empty list)
    HIP_TRY(c, hipMemsetAsync(sm.withdraw.list.n, 0, 4, c->stream));
    std::memset(sm.withdraw.h_done, 0, sizeof(WithdrawDone));
  }
  if (sm.max_depart) {  // (an empty list)
    HIP_TRY(c, hipMemsetAsync(sm.depart.list.n, 0, 4, c->stream));
    std::memset(sm.depart.h_done, 0, sizeof(DepartDone));
  }
  if (sm.quota.on) {  // (every slot of the table free; the settings follow at the next tick)
    HIP_TRY(c, hipMemsetAsync(sm.quota.d.p, 0, sm.quota.d.cap, c->stream));
    HIP_TRY(c, hipMemsetAsync(sm.quota.fd.p, 0, sm.quota.fd.cap, c->stream));  // (ask[] and the sums clear)
    std::memset(sm.quota.h_done, 0, sizeof(QuotaDone));
    std::memset(sm.quota.h_fres, 0, sizeof(FairResult));
    sm.quota.host.dirty = true;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  sm.active = true;
  return YDC_OK;
}

// The columns of W and of B as the open stream holds them, listed once: device address (NULL: the
// mode has no such column) and width in bytes. Both are compact between ticks (k_wait_compact /
// k_rpc_settle and k_book_commit leave them packed), so whoever carries them copies entries [0, n) of
// every column as they lie. The order is the snapshot's; the other side of a pairing lists the same.
struct StateCol {
  void* p;
  size_t width;
};
constexpr size_t kWCols = 8, kBCols = 4;
std::array<StateCol, kWCols> w_cols(const ydc_context::Stream& sm) {
  return {{{sm.wq.deadline, 8}, {sm.wq.tag, 8}, {sm.wl.w_for, 8} /* with leases */, {sm.wq.env, 4}, {sm.wq.minv, 4},
           {sm.wq.ip, 4}, {sm.rw.n_imm, 4} /* rpc mode */, {sm.rw.n_pre, 4}}};
}
std::array<StateCol, kBCols> b_cols(const ydc_context::Stream& sm) {
  return {{{sm.book.bk.grant, 8}, {sm.book.bk.stid, 8}, {sm.book.bk.dkey, 8}, {sm.book.bk.servant, 4}}};
}
std::array<const uint8_t*, kWCols> w_cols(const snap::View& v) {
  return {{v.w_deadline, v.w_tag, v.w_for, v.w_env, v.w_minv, v.w_ip, v.w_nimm, v.w_npre}};
}
std::array<const uint8_t*, kBCols> b_cols(const snap::View& v) { return {{v.b_grant, v.b_stid, v.b_dkey, v.b_srv}}; }

// ydc_stream_reserve: what the next tick can observe of the stream `o`, carried into the freshly
// reset, larger `n`. L is filed again slot by slot (k_lease_rehash: the new table has other home
// slots); W and B are copied as they lie; of the small state blocks only |W|, |B| and next_id
// outlive a tick (tickets, snapshots and the tick's counters are cleared by the tick that uses
// them). Nothing of `o` is written: what simply moves to `n` is stream_regrow's.
int stream_migrate(ydc_context* c, const ydc_context::Stream& o, ydc_context::Stream& n) {
  hipStream_t st = c->stream;
  LeaseState ls_old{}, ls_new{};
  if (o.leased() && o.inspect.on) {
    // With inspection: the detail records move with their leases into columns of the new table's size.
    const size_t slots = (size_t)n.lt.mask + 1;
    HIP_TRY(c, n.d_insp_rec.reserve(slots));
    HIP_TRY(c, n.d_insp_pre.reserve(slots));
    YDC_LAUNCH(c, "k_inspect_rehash", k_inspect_rehash, dim3(ceil_div(o.lt.mask + 1, 256)), dim3(256), 0, st, o.lt, o.ls,
               o.d_insp_rec.p, o.d_insp_pre.p, n.lt, n.ls, n.d_insp_rec.p, n.d_insp_pre.p);
    HIP_TRY(c, hipGetLastError());
  } else if (o.leased()) {
    YDC_LAUNCH(c, "k_lease_rehash", k_lease_rehash, dim3(ceil_div(o.lt.mask + 1, kLeaseTile)), dim3(256), 0, st,
               o.lt, o.ls, n.lt, n.ls);
    HIP_TRY(c, hipGetLastError());
  }
  if (o.waiting()) {
    uint32_t cnt = 0;
    HIP_TRY(c, hipMemcpy(&cnt, &o.ws->count, 4, hipMemcpyDeviceToHost));
    if (cnt > o.caps.max_waiting)
      return fail(c, YDC_ERR_NOT_CONVERGED, "waiting queue of %u > max_waiting %u", cnt, o.caps.max_waiting);
    const auto from = w_cols(o), to = w_cols(n);
    for (size_t k = 0; k < kWCols; ++k)
      if (cnt && from[k].p)
        HIP_TRY(c, hipMemcpyAsync(to[k].p, from[k].p, cnt * from[k].width, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(&n.ws->count, &o.ws->count, 4, hipMemcpyDeviceToDevice, st));
  }
  if (o.max_book && n.max_book) {
    if (o.book.n > n.max_book)
      return fail(c, YDC_ERR_NOT_CONVERGED, "running-task book of %u > max_book %u", o.book.n, n.max_book);
    const auto from = b_cols(o), to = b_cols(n);
    for (size_t k = 0; o.book.n && k < kBCols; ++k)
      HIP_TRY(c, hipMemcpyAsync(to[k].p, from[k].p, o.book.n * from[k].width, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(&n.book.bks->n_entries, &o.book.bks->n_entries, 4, hipMemcpyDeviceToDevice, st));
    n.book.n = o.book.n;
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  if (o.leased()) {
    HIP_TRY(c, hipMemcpy(&ls_old, o.ls, sizeof ls_old, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&ls_new, n.ls, sizeof ls_new, hipMemcpyDeviceToHost));
    if (ls_new.n_leases != ls_old.n_leases || ls_new.next_id != ls_old.next_id)
      return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u of %u leases moved (next_id %llu of %llu)",
                  ls_new.n_leases, ls_old.n_leases, ls_new.next_id, ls_old.next_id);
  }
  // The host's mirrors: |W|, rows(W), |L|, the last tick's clock, the tick number the report stamps
  // are taken from, the servants' report marks, and what the stream has learnt about its passes.
  n.n_waiting = o.n_waiting;
  n.n_wait_rows = o.n_wait_rows;
  n.n_leases = o.n_leases;
  n.last_now = o.last_now;
  n.lease_tick = o.lease_tick;
  n.rep_once = o.rep_once;
  n.want_passes = o.want_passes;
  return YDC_OK;
}

int stream_begin(ydc_context* c, const ydc_stream_caps& k) {
  if (!c || !k.max_tasks) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = stream_caps_check(c, YDC_ERR_CAPACITY, k, 0)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  stream_release(c);
  if (int rc = stream_alloc(c, c->stream_mode, k, 0, 0, 0, 0)) return rc;
  return stream_reset(c, c->stream_mode);
}

// The open stream in a second, larger set of buffers (ydc_stream_reserve, ydc_stream_book_begin,
// ydc_stream_withdraw_begin, ydc_stream_quota_begin, ydc_stream_depart_begin). quota: Stream::Quota::code.
int stream_regrow(ydc_context* c, const ydc_stream_caps& k, uint32_t max_book, uint32_t max_withdraw, uint32_t quota,
                  uint32_t max_depart) {
  auto& sm = c->stream_mode;
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // A second set of buffers, filled from the first, which is released only once that has worked:
  // after any failure the stream is as it was.
  ydc_context::Stream grown;
  int rc = stream_alloc(c, grown, k, max_book, max_withdraw, quota, max_depart);
  if (rc == YDC_OK) rc = stream_reset(c, grown);
  if (rc == YDC_OK) rc = stream_migrate(c, sm, grown);
  if (rc != YDC_OK) {
    stream_release(grown);
    return rc;
  }
  // What is sized by the registry, not by the stream, moves as it is.
  grown.d_rep_tick = std::move(sm.d_rep_tick);
  grown.alive = std::move(sm.alive);      // (a pending staging goes along)
  grown.inspect = std::move(sm.inspect);  // (the detail records have moved already: stream_migrate)
  grown.book.staged = std::move(sm.book.staged);
  grown.withdraw.host = std::move(sm.withdraw.host);  // (a pending staging and the last result go along)
  grown.depart.host = std::move(sm.depart.host);      // (likewise)
  grown.quota.host = std::move(sm.quota.host);        // (the settings and the last result go along)
  grown.quota.host.dirty = true;                      // (... and the new device copy has to follow them)
  grown.quota.host.table_dirty = false;
  grown.usage = std::move(sm.usage);  // (keyed by requestor: the table, its totals and its clock go along)
  std::swap(sm, grown);
  stream_release(grown);  // (the old buffers and the old captures; sm.stale: the step is captured again)
  return YDC_OK;
}

}  // namespace

extern "C" {

int ydc_stream_begin(ydc_context* c, uint32_t max_updates, uint32_t max_releases,
                     uint32_t max_tasks) {
  return stream_begin(c, ydc_stream_caps{max_updates, max_releases, max_tasks, 0, 0, 0, 0, 0, 0, 0});
}

int ydc_stream_begin_waiting(ydc_context* c, uint32_t max_updates, uint32_t max_releases,
                             uint32_t max_tasks, uint32_t max_waiting) {
  if (!c || !max_waiting) return YDC_ERR_INVALID_ARGUMENT;
  return stream_begin(c, ydc_stream_caps{max_updates, max_releases, max_tasks, 0, max_waiting, 0, 0, 0, 0, 0});
}

int ydc_stream_caps_get(ydc_context* c, ydc_stream_caps* out) {
  if (!c || !out || !c->stream_mode.active) return YDC_ERR_INVALID_ARGUMENT;
  *out = c->stream_mode.caps;
  return YDC_OK;
}

int ydc_stream_reserve(ydc_context* c, const ydc_stream_caps* want) {
  if (!c || !want) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_reserve: no stream is open");
  if (!sm.waiting() && !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_reserve: a stream begun with ydc_stream_begin keeps no state "
                "on the device, and its ydc_stream_buffers_get pointers stay valid until ydc_stream_end");
  if (const char* why = stream_caps_foreign(sm.caps, *want))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_reserve: %s", why);
  const ydc_stream_caps k = stream_caps_grown(sm.caps, *want);  // (growth only)
  if (int rc = stream_caps_check(c, YDC_ERR_INVALID_ARGUMENT, k, sm.max_book)) return rc;
  if (!std::memcmp(&k, &sm.caps, sizeof k)) return YDC_OK;  // (nothing to do: the captured step stays)
  return stream_regrow(c, k, sm.max_book, sm.max_withdraw, sm.quota.code(), sm.max_depart);
}

}  // extern "C"

namespace {

// ---- the servants' expiry column (servant_alive.h) ----

// A device column with a row per servant of the registry, `have` of them filed: room for `want`
// rows, the filed ones kept, the rows it gains set to `fill`. The context's stream is idle.
template <typename T>
int fit_rows(ydc_context* c, DevBuf<T>& col, uint32_t have, uint32_t want, T fill) {
  if (want > col.cap) {
    DevBuf<T> bigger;
    HIP_TRY(c, bigger.reserve((size_t)want + want / 2 + 1024));
    if (have) HIP_TRY(c, hipMemcpy(bigger.p, col.p, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice));
    col = std::move(bigger);
  }
  const std::vector<T> rows(want - have, fill);
  HIP_TRY(c, hipMemcpy(col.p + have, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice));
  return YDC_OK;
}

// discovered_at and ever_assigned have a row for every servant of the registry; rows they gain were
// discovered at `when` and have been assigned nothing (task_dispatcher.cc:208).
int inspect_fit(ydc_context* c, int64_t when) {
  auto& sm = c->stream_mode;
  auto& in = sm.inspect;
  const uint32_t S = c->reg.n;
  if (S < in.n) in.n = S;
  if (S == in.n) return YDC_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = fit_rows(c, in.disc, in.n, S, when)) return rc;
  if (int rc = fit_rows(c, in.ever, in.n, S, 0ull)) return rc;
  in.n = S;
  sm.stale = true;  // (a captured step holds the count column's address and its row count)
  return YDC_OK;
}

// E has a row for every servant of the registry; rows it gains start at "never".
int alive_fit(ydc_context* c) {
  auto& sm = c->stream_mode;
  auto& al = sm.alive;
  const uint32_t S = c->reg.n;
  if (S < al.n) al.n = S;
  if (S == al.n) return YDC_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int64_t* was = al.col.p;
  if (int rc = fit_rows(c, al.col, al.n, S, kAliveNever)) return rc;
  if (al.col.p != was) sm.stale = true;  // (a captured step holds the column's address)
  al.n = S;
  return YDC_OK;
}

// n heartbeats' expiries into E now (k_alive_beat on a device copy of the two columns).
int alive_file(ydc_context* c, const uint32_t* idx, const int64_t* expires, uint32_t n) {
  auto& sm = c->stream_mode;
  if (!n) return YDC_OK;
  HIP_TRY(c, sm.alive.d_idx.reserve(n));
  HIP_TRY(c, sm.alive.d_stage.reserve(n));
  HIP_TRY(c, hipMemcpy(sm.alive.d_idx.p, idx, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(sm.alive.d_stage.p, expires, (size_t)n * 8, hipMemcpyHostToDevice));
  YDC_LAUNCH(c, "k_alive_beat", k_alive_beat, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, sm.alive.d_idx.p,
             sm.alive.d_stage.p, n, sm.alive.n, sm.alive.col.p);
  HIP_TRY(c, hipGetLastError());
  return YDC_OK;
}

// The alarm: the rows with E < now, ascending, in alive.due[0, *n_due); alive.bound exact (the
// minimum over the rows that stay).
int alive_due(ydc_context* c, int64_t now, uint32_t* n_due) {
  auto& sm = c->stream_mode;
  *n_due = 0;
  ++sm.alive.alarms;
  if (!sm.alive.n) {
    sm.alive.bound = kAliveNever;
    return YDC_OK;
  }
  HIP_TRY(c, sm.alive.d_state.reserve(1));
  if (sm.alive.due.cap < (size_t)sm.alive.n * 4)
    HIP_TRY(c, sm.alive.due.reserve(((size_t)sm.alive.n + sm.alive.n / 2 + 1024) * 4));
  AliveState st{kAliveNever, 0, 0, 0, 0};
  HIP_TRY(c, hipMemcpy(sm.alive.d_state.p, &st, sizeof st, hipMemcpyHostToDevice));
  YDC_LAUNCH(c, "k_alive_due", k_alive_due, dim3(ceil_div(sm.alive.n, 256)), dim3(256), 0, c->stream, sm.alive.col.p,
             sm.alive.n, now, sm.alive.d_state.p, (uint32_t*)sm.alive.due.z);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(&st, sm.alive.d_state.p, sizeof st, hipMemcpyDeviceToHost));
  if (st.n_due > sm.alive.n) return fail(c, YDC_ERR_NOT_CONVERGED, "%u of %u servants due", st.n_due, sm.alive.n);
  uint32_t* due = (uint32_t*)sm.alive.due.p;
  std::sort(due, due + st.n_due);
  sm.alive.bound = st.min_expires;
  *n_due = st.n_due;
  return YDC_OK;
}

// Behind the step of a tick that took the removal route: the parked leases erased, and the tick's
// outcome block corrected — an orphan is neither a lease any more nor one that expired.
int alive_orphans(ydc_context* c) {
  auto& sm = c->stream_mode;
  YDC_LAUNCH(c, "k_alive_orphans", k_alive_orphans, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream,
             sm.lt, sm.ls, sm.alive.d_state.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  AliveState st{};
  HIP_TRY(c, hipMemcpy(&st, sm.alive.d_state.p, sizeof st, hipMemcpyDeviceToHost));
  sm.h_lout->n_leases -= std::min(sm.h_lout->n_leases, st.n_orphans);
  sm.h_lout->expired -= std::min(sm.h_lout->expired, st.n_late);
  sm.alive.orphans = st.n_orphans;
  return YDC_OK;
}

// A removal tick that ends in an error before its ending ran: the parked leases must not outlive it
// (they would count in |L| and show in ydc_stream_leases_get with a servant no registry has). The
// error that is being returned keeps its text; |L| is read back from the device.
void alive_orphans_after_error(ydc_context* c) {
  auto& sm = c->stream_mode;
  if (!sm.alive.d_state.p) return;
  (void)hipStreamSynchronize(c->stream);
  hipLaunchKernelGGL(k_alive_orphans, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream, sm.lt, sm.ls,
                     sm.alive.d_state.p);
  (void)hipStreamSynchronize(c->stream);
  AliveState st{};
  if (hipMemcpy(&st, sm.alive.d_state.p, sizeof st, hipMemcpyDeviceToHost) == hipSuccess) sm.alive.orphans = st.n_orphans;
  (void)hipMemcpy(&sm.n_leases, &sm.ls->n_leases, 4, hipMemcpyDeviceToHost);
}

// A row number after the removal of removed[0, n) (ascending); a removed row itself: kRemovedRow.
uint32_t alive_renumber(const uint32_t* removed, uint32_t n, uint32_t s) {
  const uint32_t before = (uint32_t)(std::lower_bound(removed, removed + n, s) - removed);
  return before < n && removed[before] == s ? kRemovedRow : s - before;
}

}  // namespace

extern "C" {

int ydc_stream_book_begin(ydc_context* c, uint32_t max_book) {
  if (!c || !max_book) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_book_begin: no leased, waiting-and-leased or rpc stream is open");
  if (int rc = stream_caps_check(c, YDC_ERR_INVALID_ARGUMENT, sm.caps, max_book)) return rc;
  if (max_book <= sm.max_book) return YDC_OK;  // (nothing to do: the captured step stays)
  return stream_regrow(c, ydc_stream_caps(sm.caps), max_book, sm.max_withdraw, sm.quota.code(), sm.max_depart);  // (a copy: regrow replaces the stream)
}

int ydc_stream_book_stage(ydc_context* c, const uint64_t* servant_task_id, const uint64_t* digest_key,
                          uint32_t n_ids) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_book)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_book_stage: the stream has no running-task book");
  if (n_ids > sm.caps.max_report_ids)
    return fail(c, YDC_ERR_CAPACITY, "%u staged ids > max_report_ids %u", n_ids, sm.caps.max_report_ids);
  sm.book.staged.stid.assign(n_ids, 0);
  sm.book.staged.dkey.assign(n_ids, 0);
  if (servant_task_id) std::copy_n(servant_task_id, n_ids, sm.book.staged.stid.begin());
  if (digest_key) std::copy_n(digest_key, n_ids, sm.book.staged.dkey.begin());
  sm.book.staged.on = true;
  return YDC_OK;
}

int ydc_stream_withdraw_begin(ydc_context* c, uint32_t max_withdraw) {
  if (!c || !max_withdraw) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.waiting())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_withdraw_begin: no waiting, waiting-and-leased or rpc stream is open");
  if (max_withdraw > (1u << 30))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "max_withdraw %u out of range (1 .. 2^30)", max_withdraw);
  if (max_withdraw <= sm.max_withdraw) return YDC_OK;  // (nothing to do: the captured step stays)
  return stream_regrow(c, ydc_stream_caps(sm.caps), sm.max_book, max_withdraw, sm.quota.code(), sm.max_depart);  // (a copy: regrow replaces the stream)
}

int ydc_stream_withdraw_stage(ydc_context* c, const uint64_t* tags, uint32_t n) {
  if (!c || (n && !tags)) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_withdraw)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_withdraw_stage: the stream withdraws nothing "
                "(ydc_stream_withdraw_begin)");
  if (n > sm.max_withdraw) return fail(c, YDC_ERR_CAPACITY, "%u staged tags > max_withdraw %u", n, sm.max_withdraw);
  auto& w = sm.withdraw.host;
  w.tags.assign(tags, tags + n);
  w.staged = n != 0;
  return YDC_OK;
}

int ydc_stream_withdraw_result(ydc_context* c, uint32_t* out_count, uint32_t cap, uint32_t* out_n,
                               uint32_t* out_n_withdrawn) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_withdraw)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_withdraw_result: the stream withdraws nothing "
                "(ydc_stream_withdraw_begin)");
  const auto& w = sm.withdraw.host;
  const uint32_t n = (uint32_t)w.place.size();
  *out_n = n;
  if (cap < n) return fail(c, YDC_ERR_CAPACITY, "%u staged tags > cap %u", n, cap);
  if (n && !out_count) return YDC_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; ++i) out_count[i] = w.counts[w.place[i]];
  if (out_n_withdrawn) *out_n_withdrawn = std::accumulate(w.counts.begin(), w.counts.end(), 0u);
  return YDC_OK;
}

int ydc_stream_depart_begin(ydc_context* c, uint32_t max_depart) {
  if (!c || !max_depart) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_depart_begin: no leased, waiting-and-leased or rpc stream is open");
  if (!sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_depart_begin: inspection is off, so no lease says whose it is "
                "(ydc_stream_inspect_begin)");
  if (max_depart > (1u << 24))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "max_depart %u out of range (1 .. 2^24)", max_depart);
  if (max_depart <= sm.max_depart) return YDC_OK;  // (nothing to do: the captured step stays)
  return stream_regrow(c, ydc_stream_caps(sm.caps), sm.max_book, sm.max_withdraw, sm.quota.code(), max_depart);  // (a copy: regrow replaces the stream)
}

int ydc_stream_depart_stage(ydc_context* c, const uint32_t* requestor_ip, uint32_t n) {
  if (!c || (n && !requestor_ip)) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_depart)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_depart_stage: the stream dismisses nobody "
                "(ydc_stream_depart_begin)");
  if (n > sm.max_depart) return fail(c, YDC_ERR_CAPACITY, "%u staged requestors > max_depart %u", n, sm.max_depart);
  auto& d = sm.depart.host;
  d.ips.assign(requestor_ip, requestor_ip + n);
  d.staged = n != 0;
  return YDC_OK;
}

int ydc_stream_depart_result(ydc_context* c, ydc_depart_count* out, uint32_t cap, uint32_t* out_n,
                             uint32_t* out_leases_freed, uint32_t* out_n_withdrawn) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_depart)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_depart_result: the stream dismisses nobody "
                "(ydc_stream_depart_begin)");
  const auto& d = sm.depart.host;
  const uint32_t n = (uint32_t)d.place.size();
  *out_n = n;
  if (cap < n) return fail(c, YDC_ERR_CAPACITY, "%u staged requestors > cap %u", n, cap);
  if (n && !out) return YDC_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; ++i) {
    const uint4& k = d.counts[d.place[i]];
    out[i] = ydc_depart_count{d.asked[i], k.x, k.y, k.z, k.w};
  }
  uint32_t leases = 0, waiting = 0;  // (each lease and entry once: over the list, not over the staging)
  for (const uint4& k : d.counts) {
    leases += k.x;
    waiting += k.z;
  }
  if (out_leases_freed) *out_leases_freed = leases;
  if (out_n_withdrawn) *out_n_withdrawn = waiting;
  return YDC_OK;
}

int ydc_stream_quota_begin(ydc_context* c, uint32_t max_overrides) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.waiting() || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_begin: no waiting-and-leased or rpc stream is open");
  if (!sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_begin: inspection is off, so no lease says whose it is "
                "(ydc_stream_inspect_begin)");
  if (max_overrides > (1u << 24))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "max_overrides %u out of range (0 .. 2^24)", max_overrides);
  // (a servant index is below the context's bound of servants: none may be YDC_IDX_OVER_QUOTA)
  const uint32_t bound = c->max_servants ? c->max_servants : YDC_IDX_WITHDRAWN;
  if (bound > YDC_IDX_OVER_QUOTA)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_begin: a context of up to %u servants could answer index "
                "%u, which is YDC_IDX_OVER_QUOTA (give ydc_create a max_servants)", bound, YDC_IDX_OVER_QUOTA);
  if (sm.quota.on && max_overrides <= sm.quota.max_overrides) return YDC_OK;  // (nothing to do: the captured step stays)
  return stream_regrow(c, ydc_stream_caps(sm.caps), sm.max_book, sm.max_withdraw, max_overrides + 1, sm.max_depart);  // (a copy: regrow replaces the stream)
}

int ydc_stream_quota_set(ydc_context* c, uint32_t default_cap, const uint32_t* requestor_ip, const uint32_t* cap,
                         uint32_t n) {
  if (!c || (n && (!requestor_ip || !cap))) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.quota.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_set: the stream has no quota (ydc_stream_quota_begin)");
  if (n > sm.quota.max_overrides)
    return fail(c, YDC_ERR_CAPACITY, "%u overrides > max_overrides %u", n, sm.quota.max_overrides);
  // Sorted by requestor (the kernels search the list); a requestor named twice is refused.
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return requestor_ip[a] < requestor_ip[b]; });
  for (uint32_t i = 1; i < n; ++i)
    if (requestor_ip[order[i]] == requestor_ip[order[i - 1]])
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_set: requestor %u has two overrides", requestor_ip[order[i]]);
  auto& h = sm.quota.host;
  h.default_cap = default_cap;
  h.ip.resize(n);
  h.cap.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    h.ip[i] = requestor_ip[order[i]];
    h.cap[i] = cap[order[i]];
  }
  h.dirty = true;  // (the device copy follows in front of the next accepted tick)
  return YDC_OK;
}

int ydc_stream_quota_fair(ydc_context* c, uint32_t mode, uint32_t pool, uint32_t floor_cap) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.quota.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_fair: the stream has no quota (ydc_stream_quota_begin)");
  if (mode > YDC_FAIR_FIXED) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_fair: mode %u is unknown", mode);
  if (mode == YDC_FAIR_REGISTRY && pool == 0)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_fair: 0 percent of the registry's capacity");
  auto& h = sm.quota.host;
  // (between off and on the step launches other kernels: captured again at the next tick; numbers alone are read from HBM)
  if ((h.fair_mode == kFairOff) != (mode == kFairOff)) sm.stale = true;
  h.fair_mode = mode;
  h.fair_pool = pool;
  h.fair_floor = floor_cap;
  h.dirty = true;  // (the device copy follows in front of the next accepted tick)
  return YDC_OK;
}

int ydc_stream_quota_fair_result(ydc_context* c, ydc_fair_result* out) {
  static_assert(sizeof(ydc_fair_result) == sizeof(FairResult), "ydc_fair_result");
  if (!c || !out) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.quota.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_fair_result: the stream has no quota (ydc_stream_quota_begin)");
  std::memcpy(out, &sm.quota.host.fair_res, sizeof *out);
  return YDC_OK;
}

int ydc_fair_level(const uint32_t* held, const uint32_t* asked, const uint32_t* fixed_cap, uint32_t n, uint64_t others,
                   uint64_t pool, uint32_t* out_level) {
  if (!out_level || (n && (!held || !asked))) return YDC_ERR_INVALID_ARGUMENT;
  *out_level = fair_level(held, asked, fixed_cap, n, others, pool);
  return YDC_OK;
}

int ydc_stream_quota_result(ydc_context* c, uint32_t* out_immediate, uint32_t* out_prefetch, uint32_t cap,
                            uint32_t* out_n, uint32_t* out_rows_clipped, uint32_t* out_n_refused) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.quota.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_quota_result: the stream has no quota (ydc_stream_quota_begin)");
  const auto& h = sm.quota.host;
  const uint32_t n = (uint32_t)h.imm.size();
  *out_n = n;
  if (cap < n) return fail(c, YDC_ERR_CAPACITY, "%u new requests > cap %u", n, cap);
  if (n && (!out_immediate || (sm.rpc() && !out_prefetch))) return YDC_ERR_INVALID_ARGUMENT;
  if (n) std::memcpy(out_immediate, h.imm.data(), (size_t)n * 4);
  if (n && out_prefetch) {
    if (sm.rpc()) std::memcpy(out_prefetch, h.pre.data(), (size_t)n * 4);
    else std::memset(out_prefetch, 0, (size_t)n * 4);
  }
  if (out_rows_clipped) *out_rows_clipped = h.rows_clipped;
  if (out_n_refused) *out_n_refused = h.n_refused;
  return YDC_OK;
}

int ydc_stream_book_get(ydc_context* c, uint32_t* out_servant_idx, uint64_t* out_task_grant_id,
                        uint64_t* out_servant_task_id, uint64_t* out_digest_key, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.max_book)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_book_get: the stream has no running-task book");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t n = sm.book.n;
  *out_n = n;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u book entries > cap %u", n, cap);
  if (n && (!out_servant_idx || !out_task_grant_id || !out_servant_task_id || !out_digest_key))
    return YDC_ERR_INVALID_ARGUMENT;
  const auto from = b_cols(sm);
  void* const to[kBCols] = {out_task_grant_id, out_servant_task_id, out_digest_key, out_servant_idx};
  for (size_t k = 0; n && k < kBCols; ++k) HIP_TRY(c, hipMemcpy(to[k], from[k].p, n * from[k].width, hipMemcpyDeviceToHost));
  return YDC_OK;
}

static int outlook_enter(ydc_context* c, const char* who);  // (further down, with the outlook)

// What both read calls of the digest index do first: the outlook's refusals and its draining of the
// stream, then the index over B as B is now — built here when the one at hand is stale or there is
// none (book_index.h). *rebuilt: this call built it. A failed build leaves no index and the stream
// as it was.
static int book_index_enter(ydc_context* c, const char* who, uint32_t* rebuilt) {
  *rebuilt = 0;
  if (int rc = outlook_enter(c, who)) return rc;
  auto& sm = c->stream_mode;
  if (!sm.max_book) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the stream has no running-task book", who);
  auto& ix = sm.book.index;
  if (ix.valid) return YDC_OK;
  const uint32_t n = sm.book.n, slots = book_index_slots(n);
  const size_t o_last = (size_t)slots * 8, o_cnt = o_last + (size_t)slots * 4, o_side = o_cnt + (size_t)slots * 4;
  HIP_TRY(c, ix.d.reserve(o_side + 8));
  uint8_t* const b = ix.d.p;
  ix.ix = BookIndex{(unsigned long long*)b, (uint32_t*)(b + o_last), (uint32_t*)(b + o_cnt), (uint32_t*)(b + o_side),
                    slots - 1};
  HIP_TRY(c, hipMemsetAsync(b, 0xFF, o_last, c->stream));               // every slot free
  HIP_TRY(c, hipMemsetAsync(b + o_last, 0, o_side + 8 - o_last, c->stream));  // last1 | cnt | side
  if (n)
    YDC_LAUNCH(c, "k_book_index_build", k_book_index_build, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream,
               sm.book.bk.dkey, n, ix.ix);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ix.valid = true;
  *rebuilt = 1;
  return YDC_OK;
}

int ydc_stream_book_find(ydc_context* c, const uint64_t* digest_key, uint32_t n, ydc_book_hit* out,
                         uint32_t* out_rebuilt) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (out_rebuilt) *out_rebuilt = 0;
  if (n > (1u << 24))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_book_find: %u queries > 2^24 in one call", n);
  if (n && (!digest_key || !out))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_book_find: %u queries without their columns", n);
  uint32_t rebuilt = 0;
  const int rc = book_index_enter(c, "ydc_stream_book_find", &rebuilt);
  if (out_rebuilt) *out_rebuilt = rebuilt;
  if (rc || !n) return rc;
  auto& sm = c->stream_mode;
  auto& ix = sm.book.index;
  static_assert(sizeof(ydc_book_hit) == sizeof(BookHit), "ydc_book_hit");
  HIP_TRY(c, ix.q.reserve(n));
  HIP_TRY(c, ix.res.reserve(n));
  HIP_TRY(c, hipMemcpy(ix.q.p, digest_key, (size_t)n * 8, hipMemcpyHostToDevice));
  YDC_LAUNCH(c, "k_book_index_find", k_book_index_find, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, ix.q.p, n, ix.ix,
             sm.book.bk, sm.book.n, ix.res.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, ix.res.p, (size_t)n * sizeof(BookHit), hipMemcpyDeviceToHost));
  return YDC_OK;
}

int ydc_stream_book_distinct(ydc_context* c, uint32_t* out_servant_idx, uint64_t* out_task_grant_id,
                             uint64_t* out_servant_task_id, uint64_t* out_digest_key, uint32_t* out_count,
                             uint32_t cap, uint32_t* out_n, uint32_t* out_rebuilt) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  if (out_rebuilt) *out_rebuilt = 0;
  uint32_t rebuilt = 0;
  const int rc = book_index_enter(c, "ydc_stream_book_distinct", &rebuilt);
  if (out_rebuilt) *out_rebuilt = rebuilt;
  if (rc) return rc;
  auto& sm = c->stream_mode;
  auto& ix = sm.book.index;
  const uint32_t n = sm.book.n;
  *out_n = 0;
  if (!n) return YDC_OK;
  // The pass's own ticket, count and look-back words | the five output columns, |B| rows each.
  const uint32_t tiles = ceil_div(n, kBookTile);
  size_t off = 0;
  const size_t o_state = section(&off, sizeof(BookDistinctState)), o_lb = section(&off, (size_t)tiles * 8);
  const size_t clear = off;
  const size_t o_gr = section(&off, (size_t)n * 8), o_st = section(&off, (size_t)n * 8), o_dk = section(&off, (size_t)n * 8);
  const size_t o_srv = section(&off, (size_t)n * 4), o_cnt = section(&off, (size_t)n * 4);
  HIP_TRY(c, ix.rows.reserve(off));
  uint8_t* const b = ix.rows.p;
  BookDistinctState* const ds = (BookDistinctState*)(b + o_state);
  const BookDistinctOut rows{(uint32_t*)(b + o_srv), (unsigned long long*)(b + o_gr), (unsigned long long*)(b + o_st),
                             (unsigned long long*)(b + o_dk), (uint32_t*)(b + o_cnt)};
  HIP_TRY(c, hipMemsetAsync(b, 0, clear, c->stream));
  YDC_LAUNCH(c, "k_book_distinct", k_book_distinct, dim3(tiles), dim3(256), 0, c->stream, sm.book.bk, n, ix.ix, ds,
             (unsigned long long*)(b + o_lb), rows);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint32_t m = 0;
  HIP_TRY(c, hipMemcpy(&m, &ds->n_rows, 4, hipMemcpyDeviceToHost));
  if (m > n) return fail(c, YDC_ERR_NOT_CONVERGED, "%u distinct keys among %u book entries", m, n);
  *out_n = m;
  if (m > cap) return fail(c, YDC_ERR_CAPACITY, "%u distinct keys > cap %u", m, cap);
  const struct {
    void* to;
    const void* from;
    size_t width;
  } cols[] = {{out_servant_idx, rows.servant, 4}, {out_task_grant_id, rows.grant, 8}, {out_servant_task_id, rows.stid, 8},
              {out_digest_key, rows.dkey, 8}, {out_count, rows.count, 4}};
  for (const auto& k : cols)
    if (k.to) HIP_TRY(c, hipMemcpy(k.to, k.from, m * k.width, hipMemcpyDeviceToHost));
  return YDC_OK;
}

int ydc_stream_alive_begin(ydc_context* c, const int64_t* expires_at, uint32_t n) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_alive_begin: no leased, waiting-and-leased or rpc stream is open");
  if (n != c->reg.n)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_alive_begin: %u expiries for %u servants", n, c->reg.n);
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int64_t* old = sm.alive.col.p;
  HIP_TRY(c, sm.alive.col.reserve((size_t)n + n / 2 + 1024));
  std::vector<int64_t> col(n, kAliveNever);
  if (expires_at) std::copy_n(expires_at, n, col.begin());
  if (n) HIP_TRY(c, hipMemcpy(sm.alive.col.p, col.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  sm.alive.bound = kAliveNever;
  for (int64_t e : col) sm.alive.bound = std::min(sm.alive.bound, e);
  sm.alive.n = n;
  if (!sm.alive.on || old != sm.alive.col.p) sm.stale = true;  // (the step gains k_alive_beat: captured again)
  sm.alive.on = true;
  return YDC_OK;
}

int ydc_stream_alive_stage(ydc_context* c, const int64_t* upd_expires_at, uint32_t n_upd) {
  if (!c || (n_upd && !upd_expires_at)) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.alive.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_alive_stage: the stream keeps no servant expiries");
  if (n_upd > sm.caps.max_updates)
    return fail(c, YDC_ERR_CAPACITY, "%u staged expiries > max_updates %u", n_upd, sm.caps.max_updates);
  sm.alive.stage.assign(upd_expires_at, upd_expires_at + n_upd);
  sm.alive.staged = true;
  return YDC_OK;
}

int ydc_stream_alive_removed(ydc_context* c, uint32_t* out_idx, uint32_t cap, uint32_t* out_n,
                             uint32_t* out_n_orphans) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.alive.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_alive_removed: the stream keeps no servant expiries");
  const uint32_t n = (uint32_t)sm.alive.removed.size();
  *out_n = n;
  if (out_n_orphans) *out_n_orphans = sm.alive.orphans;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u removed servants > cap %u", n, cap);
  if (n && !out_idx) return YDC_ERR_INVALID_ARGUMENT;
  if (n) std::memcpy(out_idx, sm.alive.removed.data(), (size_t)n * 4);
  return YDC_OK;
}

int ydc_stream_alive_get(ydc_context* c, int64_t* out_expires_at, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.alive.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_alive_get: the stream keeps no servant expiries");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = alive_fit(c)) return rc;
  const uint32_t n = sm.alive.n;
  *out_n = n;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u servant expiries > cap %u", n, cap);
  if (n && !out_expires_at) return YDC_ERR_INVALID_ARGUMENT;
  if (n) HIP_TRY(c, hipMemcpy(out_expires_at, sm.alive.col.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return YDC_OK;
}

// Tests and tools (not part of the ABI): the host's lower bound of min(E), the ticks that launched
// k_alive_due so far and the servants the ticks removed so far.
int ydc_debug_alive(ydc_context* c, int64_t* out_bound, uint64_t* out_alarms, uint64_t* out_removals) {
  if (!c || !c->stream_mode.active || !c->stream_mode.alive.on) return YDC_ERR_INVALID_ARGUMENT;
  if (out_bound) *out_bound = c->stream_mode.alive.bound;
  if (out_alarms) *out_alarms = c->stream_mode.alive.alarms;
  if (out_removals) *out_removals = c->stream_mode.alive.removals;
  return YDC_OK;
}

// ---- inspection (stream_inspect.h) ----

int ydc_stream_inspect_begin(ydc_context* c, const int64_t* discovered_at, const uint64_t* ever_assigned, uint32_t n) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_begin: no leased, waiting-and-leased or rpc stream is open");
  if (n != c->reg.n)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_begin: %u rows for %u servants", n, c->reg.n);
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, sm.inspect.disc.reserve((size_t)n + n / 2 + 1024));
  HIP_TRY(c, sm.inspect.ever.reserve((size_t)n + n / 2 + 1024));
  const size_t slots = (size_t)sm.lt.mask + 1;
  if (!sm.inspect.on) {
    HIP_TRY(c, sm.d_insp_rec.reserve(slots));
    HIP_TRY(c, sm.d_insp_pre.reserve(slots));
  }
  std::vector<int64_t> disc(n, sm.last_now == INT64_MIN ? 0 : sm.last_now);
  std::vector<unsigned long long> ever(n, 0);
  if (discovered_at) std::copy_n(discovered_at, n, disc.begin());
  if (ever_assigned) std::copy_n(ever_assigned, n, ever.begin());
  if (n) {
    HIP_TRY(c, hipMemcpy(sm.inspect.disc.p, disc.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(sm.inspect.ever.p, ever.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  }
  if (!sm.inspect.on) {  // (the leases L holds were granted without details)
    YDC_LAUNCH(c, "k_inspect_fill", k_inspect_fill, dim3(ceil_div((uint32_t)slots, 256)), dim3(256), 0, c->stream,
               sm.d_insp_rec.p, sm.d_insp_pre.p, (uint32_t)slots);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  sm.inspect.n = n;
  sm.inspect.on = true;
  ++sm.inspect.epoch;
  sm.stale = true;  // (the step's granting pass changes, and it holds the columns' addresses: captured again)
  return YDC_OK;
}

int ydc_stream_inspect_load(ydc_context* c, const uint64_t* task_id, const int64_t* started_at, const uint32_t* env_id,
                            const uint32_t* requestor_ip, const uint8_t* prefetch, uint32_t n) {
  if (!c || (n && !task_id)) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_load: the stream has no inspection");
  if (n > sm.n_leases) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_load: %u records for %u leases", n, sm.n_leases);
  if (!n) return YDC_OK;
  {
    std::vector<uint64_t> sorted(task_id, task_id + n);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    if (dup != sorted.end())
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_load: task %llu appears twice", (unsigned long long)*dup);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevBuf<unsigned long long> d_id;
  DevBuf<int64_t> d_at;
  DevBuf<uint32_t> d_slot, d_env, d_ip, d_miss;
  DevBuf<uint8_t> d_pre;
  HIP_TRY(c, d_id.reserve(n));
  HIP_TRY(c, d_slot.reserve(n));
  HIP_TRY(c, d_miss.reserve(1));
  HIP_TRY(c, hipMemcpy(d_id.p, task_id, (size_t)n * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemset(d_miss.p, 0, 4));
  YDC_LAUNCH(c, "k_inspect_find", k_inspect_find, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, sm.lt, sm.ls, d_id.p, n,
             d_slot.p, d_miss.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint32_t missing = 0;
  HIP_TRY(c, hipMemcpy(&missing, d_miss.p, 4, hipMemcpyDeviceToHost));
  if (missing) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_load: %u of %u ids are no lease", missing, n);
  if (started_at) {
    HIP_TRY(c, d_at.reserve(n));
    HIP_TRY(c, hipMemcpy(d_at.p, started_at, (size_t)n * 8, hipMemcpyHostToDevice));
  }
  if (env_id) {
    HIP_TRY(c, d_env.reserve(n));
    HIP_TRY(c, hipMemcpy(d_env.p, env_id, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (requestor_ip) {
    HIP_TRY(c, d_ip.reserve(n));
    HIP_TRY(c, hipMemcpy(d_ip.p, requestor_ip, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (prefetch) {
    HIP_TRY(c, d_pre.reserve(n));
    HIP_TRY(c, hipMemcpy(d_pre.p, prefetch, n, hipMemcpyHostToDevice));
  }
  YDC_LAUNCH(c, "k_inspect_file", k_inspect_file, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, d_slot.p, n,
             sm.lt.mask + 1, d_at.p, d_env.p, d_ip.p, d_pre.p, sm.d_insp_rec.p, sm.d_insp_pre.p);
  HIP_TRY(c, hipGetLastError());
  ++sm.inspect.epoch;
  if (sm.usage.on) sm.usage.fresh += n;  // (the filed records may name requestors its table has not met)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return YDC_OK;
}

int ydc_stream_inspect_servants(ydc_context* c, int64_t* out_discovered_at, uint64_t* out_ever_assigned,
                                uint32_t* out_running_tasks, uint32_t* out_capacity_available, uint32_t cap,
                                uint32_t* out_n, ydc_stream_totals* out_totals) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_servants: the stream has no inspection");
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = inspect_fit(c, sm.last_now == INT64_MIN ? 0 : sm.last_now)) return rc;
  const uint32_t n = sm.inspect.n;
  *out_n = n;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u servants > cap %u", n, cap);
  HIP_TRY(c, sm.inspect.avail.reserve(n));
  HIP_TRY(c, sm.inspect.sums.reserve(1));
  InspectSums sums{0, 0, 0};
  HIP_TRY(c, hipMemcpy(sm.inspect.sums.p, &sums, sizeof sums, hipMemcpyHostToDevice));
  if (n) {
    YDC_LAUNCH(c, "k_inspect_servants", k_inspect_servants, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, c->d_nproc.p,
               c->d_load.p, c->d_max_tasks.p, c->d_running.p, c->d_flags.p, n, sm.inspect.avail.p, sm.inspect.sums.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (out_discovered_at) HIP_TRY(c, hipMemcpy(out_discovered_at, sm.inspect.disc.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (out_ever_assigned) HIP_TRY(c, hipMemcpy(out_ever_assigned, sm.inspect.ever.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (out_running_tasks) HIP_TRY(c, hipMemcpy(out_running_tasks, c->d_running.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (out_capacity_available)
      HIP_TRY(c, hipMemcpy(out_capacity_available, sm.inspect.avail.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&sums, sm.inspect.sums.p, sizeof sums, hipMemcpyDeviceToHost));
  }
  if (out_totals) {
    // (task_dispatcher.cc:604-612, u64 arithmetic modulo 2^64)
    const uint64_t left = (uint64_t)sums.capacity - (uint64_t)sums.running - (uint64_t)sums.unavailable;
    *out_totals = ydc_stream_totals{n, sums.running, sums.capacity, (uint64_t)std::max<int64_t>((int64_t)left, 0),
                                    sums.unavailable};
  }
  return YDC_OK;
}

int ydc_stream_inspect_tasks(ydc_context* c, uint64_t* out_task_id, uint32_t* out_servant_idx, int64_t* out_expires_at,
                             uint8_t* out_zombie, int64_t* out_started_at, uint32_t* out_env_id,
                             uint32_t* out_requestor_ip, uint8_t* out_prefetch, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_tasks: the stream has no inspection");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t nl = sm.n_leases;
  *out_n = nl;
  if (nl > cap) return fail(c, YDC_ERR_CAPACITY, "%u leases > cap %u", nl, cap);
  // One pass over the table; |L| records cross the bus, not 2^k slots; sorted by id here.
  const size_t pc = std::max(nl, 1u), o_cnt = (pc * 41 + 3) & ~(size_t)3;
  HIP_TRY(c, sm.inspect.pack.reserve(o_cnt + 4));
  uint8_t* d = sm.inspect.pack.p;
  const InspectPacked pk{(unsigned long long*)(d + pc * 16), (int64_t*)(d + pc * 24), (uint4*)d,
                         (uint32_t*)(d + pc * 32),            (uint32_t*)(d + pc * 36), d + pc * 40, (uint32_t)pc};
  HIP_TRY(c, hipMemsetAsync(d + o_cnt, 0, 4, c->stream));
  YDC_LAUNCH(c, "k_inspect_pack", k_inspect_pack, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream,
             sm.lt, sm.d_insp_rec.p, sm.d_insp_pre.p, pk, (uint32_t*)(d + o_cnt));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<uint8_t> h(o_cnt + 4);
  HIP_TRY(c, hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost));
  uint32_t packed = 0;
  std::memcpy(&packed, h.data() + o_cnt, 4);
  if (packed != nl) return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u live slots, |L| %u on the host", packed, nl);
  auto at = [&](size_t off, size_t width, uint32_t i, void* out) { std::memcpy(out, h.data() + off + (size_t)i * width, width); };
  std::vector<std::pair<unsigned long long, uint32_t>> order(nl);  // (id, packed position)
  for (uint32_t i = 0; i < nl; ++i) {
    at(pc * 16, 8, i, &order[i].first);
    order[i].second = i;
  }
  std::sort(order.begin(), order.end());
  for (uint32_t k = 0; k < nl; ++k) {
    const uint32_t i = order[k].second;
    uint32_t rec[4], state = 0;
    at(0, 16, i, rec);
    at(pc * 36, 4, i, &state);
    if (out_task_id) out_task_id[k] = order[k].first;
    if (out_servant_idx) at(pc * 32, 4, i, &out_servant_idx[k]);
    if (out_expires_at) at(pc * 24, 8, i, &out_expires_at[k]);
    if (out_zombie) out_zombie[k] = (state & kLeaseZombie) ? 1 : 0;
    if (out_started_at) out_started_at[k] = (int64_t)((uint64_t)rec[0] | ((uint64_t)rec[1] << 32));
    if (out_env_id) out_env_id[k] = rec[2];
    if (out_requestor_ip) out_requestor_ip[k] = rec[3];
    if (out_prefetch) out_prefetch[k] = h[pc * 40 + i];
  }
  return YDC_OK;
}

// What both read calls of the outlook refuse, and what every entry point does before it reads the
// registry: the resident kernel ended, the stream's work drained.
static int outlook_enter(ydc_context* c, const char* who) {
  auto& sm = c->stream_mode;
  if (!sm.active) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: no stream is open", who);
  if (!sm.waiting() && !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: a stream begun with ydc_stream_begin keeps no state on the device", who);
  if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: pipelined batches are outstanding", who);
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return YDC_OK;
}

int ydc_stream_outlook_get(ydc_context* c, const uint32_t* env_id, const uint32_t* min_version, uint32_t n,
                           ydc_stream_outlook* out) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (n && (!env_id || !min_version || !out))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_outlook_get: %u queries without their columns", n);
  if (int rc = outlook_enter(c, "ydc_stream_outlook_get")) return rc;
  if (!n) return YDC_OK;
  auto& sm = c->stream_mode;
  if (c->tables_dirty)
    if (int rc = rebuild_tables(c)) return rc;  // (what the next tick would do first)
  const uint32_t S = c->reg.n, C = c->tables.n_classes(), EW = c->reg.env_words, bins = 64 * EW + 1;
  const bool with_w = sm.waiting(), with_l = sm.leased() && sm.inspect.on;
  const size_t n_agg = (size_t)std::max(C, 1u) * kOutlookCols, n_res = (size_t)n * kOutlookCols;
  HIP_TRY(c, sm.outlook.agg.reserve(n_agg));
  HIP_TRY(c, sm.outlook.res.reserve(n_res));
  HIP_TRY(c, sm.outlook.q.reserve((size_t)n * 2));
  HIP_TRY(c, sm.outlook.hist.reserve((size_t)bins * 4));
  uint32_t *d_env = sm.outlook.q.p, *d_minv = d_env + n;
  uint32_t *d_hw = sm.outlook.hist.p, *d_hl = d_hw + (size_t)bins * 2;
  HIP_TRY(c, hipMemcpy(d_env, env_id, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_minv, min_version, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemsetAsync(sm.outlook.agg.p, 0, n_agg * 8, c->stream));
  HIP_TRY(c, hipMemsetAsync(d_hw, 0, (size_t)bins * 16, c->stream));
  if (S && C)
    YDC_LAUNCH(c, "k_outlook_classes", k_outlook_classes, dim3(ceil_div(S, 256)), dim3(256), 0, c->stream, c->d_nproc.p,
               c->d_load.p, c->d_max_tasks.p, c->d_running.p, c->d_flags.p, c->d_class_of.p, S, C, sm.outlook.agg.p);
  YDC_LAUNCH(c, "k_outlook_queries", k_outlook_queries, dim3(ceil_div(n, 4)), dim3(256), 0, c->stream, d_env, d_minv, n,
             c->d_cls_env.p, c->d_cls_ver.p, C, EW, sm.outlook.agg.p, sm.outlook.res.p);
  if (with_w)
    YDC_LAUNCH(c, "k_outlook_waiting", k_outlook_waiting, dim3(std::max(ceil_div(sm.n_waiting, 256), 1u)), dim3(256), 0,
               c->stream, sm.wq.env, sm.rw.n_imm, sm.rw.n_pre, sm.ws, sm.caps.max_waiting, bins, d_hw);
  if (with_l)
    YDC_LAUNCH(c, "k_outlook_leases", k_outlook_leases, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0,
               c->stream, sm.lt, sm.d_insp_rec.p, bins, d_hl);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> res(n_res);
  std::vector<uint32_t> hist((size_t)bins * 4);
  HIP_TRY(c, hipMemcpy(res.data(), sm.outlook.res.p, n_res * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(hist.data(), sm.outlook.hist.p, (size_t)bins * 16, hipMemcpyDeviceToHost));
  // The per-digest histograms fanned out to the queries (the last bin is nobody's).
  for (uint32_t q = 0; q < n; ++q) {
    const unsigned long long* r = &res[(size_t)q * kOutlookCols];
    const uint32_t e = env_id[q];
    const bool known = e < bins - 1;
    ydc_stream_outlook o{};
    o.eligible = (uint32_t)r[0];
    o.free_servants = (uint32_t)r[1];
    o.grants_available = r[2];
    o.running_tasks = r[3];
    o.max_tasks = r[4];
    o.capacity_available = r[5];
    o.waiting = with_w && known ? hist[e] : 0;
    o.waiting_rows = with_w && known ? hist[bins + e] : 0;
    o.leases = !with_l ? YDC_OUTLOOK_UNKNOWN : known ? hist[(size_t)bins * 2 + e] : 0;
    o.zombies = !with_l ? YDC_OUTLOOK_UNKNOWN : known ? hist[(size_t)bins * 3 + e] : 0;
    out[q] = o;
  }
  return YDC_OK;
}

int ydc_stream_inspect_waiting(ydc_context* c, uint64_t* out_tag, uint32_t* out_env_id, uint32_t* out_min_version,
                               uint32_t* out_requestor_ip, int64_t* out_deadline, int64_t* out_lease_for,
                               uint32_t* out_n_immediate, uint32_t* out_n_prefetch, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = outlook_enter(c, "ydc_stream_inspect_waiting")) return rc;
  auto& sm = c->stream_mode;
  uint32_t n = 0;
  if (sm.waiting()) {
    HIP_TRY(c, hipMemcpy(&n, &sm.ws->count, 4, hipMemcpyDeviceToHost));
    if (n > sm.caps.max_waiting)
      return fail(c, YDC_ERR_NOT_CONVERGED, "waiting queue of %u on the device, room for %u", n, sm.caps.max_waiting);
  }
  *out_n = n;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u waiting requests > cap %u", n, cap);
  // Entries [0, |W|) of the mode's own columns; what the mode lacks: 0 (one immediate row outside rpc mode).
  const auto from = w_cols(sm);
  void* const to[kWCols] = {out_deadline,     out_tag,         out_lease_for,  out_env_id, out_min_version,
                            out_requestor_ip, out_n_immediate, out_n_prefetch};
  for (size_t k = 0; n && k < kWCols; ++k) {
    if (!to[k]) continue;
    if (from[k].p) HIP_TRY(c, hipMemcpy(to[k], from[k].p, n * from[k].width, hipMemcpyDeviceToHost));
    else std::memset(to[k], 0, n * from[k].width);
  }
  if (!sm.rpc() && out_n_immediate) std::fill(out_n_immediate, out_n_immediate + n, 1u);
  return YDC_OK;
}

// ---- select and count over L (stream_select.h, lease_filter.h) ----

static_assert(sizeof(ydc_lease_filter) == sizeof(LeaseFilter), "ydc_lease_filter");
constexpr size_t kSelectFiltersAt = sizeof(SelectState), kSelectPackAt = kSelectFiltersAt + kSelectMaxFilters * sizeof(LeaseFilter);
static_assert(kSelectFiltersAt % 16 == 0 && kSelectPackAt % 16 == 0, "the scratch's sections hold 16-byte vectors");

// What both calls do first: the filters checked, the outlook's refusals and its draining of the
// stream, the refusals of their own; then the scratch with room for `pack_bytes` of packed rows,
// the filters in it and its state cleared (enqueued).
static int select_enter(ydc_context* c, const char* who, const ydc_lease_filter* f, uint32_t n, size_t pack_bytes) {
  for (uint32_t i = 0; i < n; ++i) {
    LeaseFilter lf;
    std::memcpy(&lf, &f[i], sizeof lf);
    if (!lease_filter_valid(lf))
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: filter %u selects 0x%x with zombie %u, prefetch %u", who, i, lf.fields,
                  lf.zombie, lf.prefetch);
  }
  if (int rc = outlook_enter(c, who)) return rc;
  auto& sm = c->stream_mode;
  if (!sm.leased()) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: a waiting stream keeps no leases", who);
  for (uint32_t i = 0; i < n; ++i)
    if ((f[i].fields & kSelRecord) && !sm.inspect.on)
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: filter %u selects by a lease's record, and inspection is off "
                  "(ydc_stream_inspect_begin)", who, i);
  if (!n) return YDC_OK;
  HIP_TRY(c, sm.select.reserve(kSelectPackAt + pack_bytes));
  uint8_t* const d = sm.select.p;
  SelectState* const st = (SelectState*)d;
  HIP_TRY(c, sm.select_h.reserve(kSelectMaxFilters * sizeof(LeaseFilter)));
  std::memcpy(sm.select_h.p, f, (size_t)n * sizeof(LeaseFilter));  // (n <= kSelectMaxFilters: both callers)
  HIP_TRY(c, hipMemcpyAsync(d + kSelectFiltersAt, sm.select_h.p, (size_t)n * sizeof(LeaseFilter), hipMemcpyHostToDevice,
                            c->stream));
  HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(SelectState), c->stream));
  HIP_TRY(c, hipMemsetAsync(&st->min_id, 0xFF, sizeof st->min_id, c->stream));
  return YDC_OK;
}

int ydc_stream_inspect_select(ydc_context* c, const ydc_lease_filter* f, uint64_t* out_task_id, uint32_t* out_servant_idx,
                              int64_t* out_expires_at, uint8_t* out_zombie, int64_t* out_started_at, uint32_t* out_env_id,
                              uint32_t* out_requestor_ip, uint8_t* out_prefetch, uint32_t cap, uint32_t* out_n,
                              uint32_t* out_matches) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (!f || !out_n || !out_matches)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_select: no filter, or nowhere to put the counts");
  auto& sm = c->stream_mode;
  // A call returns min(matches, cap) <= |L| rows, so that is the room the pack gets.
  const uint32_t room = sm.active && sm.leased() ? std::min(cap, sm.n_leases) : 0u;
  if (int rc = select_enter(c, "ydc_stream_inspect_select", f, 1, (size_t)std::max(room, 1u) * 41 + 3)) return rc;
  uint8_t* const d = sm.select.p;
  SelectState* const st = (SelectState*)d;
  const LeaseFilter* const df = (const LeaseFilter*)(d + kSelectFiltersAt);
  const uint4* const rec = sm.inspect.on ? sm.d_insp_rec.p : nullptr;
  const uint8_t* const pre = sm.inspect.on ? sm.d_insp_pre.p : nullptr;
  const dim3 grid(ceil_div(sm.lt.mask + 1, kLeaseTile)), block(256);
  // Pass 1: the matches, the smallest and the largest matching id.
  YDC_LAUNCH(c, "k_select_count", k_select_count<true>, grid, block, 0, c->stream, sm.lt, rec, pre, df, 1u, st);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  struct {
    uint32_t matches[kSelectMaxFilters];
    unsigned long long min_id, max_id;
  } head;
  static_assert(offsetof(SelectState, max_id) + 8 == sizeof head, "SelectState's head");
  HIP_TRY(c, hipMemcpy(&head, st, sizeof head, hipMemcpyDeviceToHost));
  const uint32_t matches = head.matches[0], n_out = std::min(matches, cap);
  if (matches > sm.n_leases || (matches && head.min_id > head.max_id))
    return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u matches, |L| %u on the host", matches, sm.n_leases);
  if (!n_out) {
    *out_n = 0;
    *out_matches = matches;
    return YDC_OK;
  }
  // More matches than room: the cap-th smallest matching id by a radix select over the bytes the
  // matches do not share, eight launches of which those above `top` return at once. Otherwise
  // every match is packed.
  struct {
    unsigned long long prefix;
    uint32_t rank, n_packed;
  } sel{~0ull, 0u, 0u};
  static_assert(offsetof(SelectState, n_packed) - offsetof(SelectState, prefix) == 12, "SelectState's select part");
  const bool cut = matches > cap;
  uint32_t top = 0;
  if (cut) {
    top = (63u - (uint32_t)__builtin_clzll(head.min_id ^ head.max_id)) / 8u;  // (two matches: min != max)
    sel.prefix = top >= 7 ? 0ull : head.min_id & ~((1ull << (8 * (top + 1))) - 1ull);
    sel.rank = cap;
  }
  HIP_TRY(c, hipMemcpy(&st->prefix, &sel, sizeof sel, hipMemcpyHostToDevice));
  if (cut)
    for (uint32_t b = kSelectRounds; b-- > 0;) {
      YDC_LAUNCH(c, "k_select_hist", k_select_hist, grid, block, 0, c->stream, sm.lt, rec, pre, df, b, top, st);
      YDC_LAUNCH(c, "k_select_digit", k_select_digit, dim3(1), block, 0, c->stream, b, top, st);
    }
  // The pack: n_out rows in the layout of ydc_stream_inspect_tasks' pack, sized by n_out.
  const size_t pc = n_out;
  uint8_t* const pd = d + kSelectPackAt;
  const InspectPacked pk{(unsigned long long*)(pd + pc * 16), (int64_t*)(pd + pc * 24), (uint4*)pd,
                         (uint32_t*)(pd + pc * 32),            (uint32_t*)(pd + pc * 36), pd + pc * 40, n_out};
  YDC_LAUNCH(c, "k_select_pack", k_select_pack, grid, block, 0, c->stream, sm.lt, rec, pre, df, pk, st);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(&sel, &st->prefix, sizeof sel, hipMemcpyDeviceToHost));
  if (sel.n_packed != n_out)
    return fail(c, YDC_ERR_NOT_CONVERGED, "lease select: %u rows at or below the threshold, %u expected", sel.n_packed, n_out);
  std::vector<uint8_t> h(pc * 41);
  HIP_TRY(c, hipMemcpy(h.data(), pd, h.size(), hipMemcpyDeviceToHost));
  // Sorted by id here, as ydc_stream_inspect_tasks sorts: n_out rows.
  auto at = [&](size_t off, size_t width, uint32_t i, void* out) { std::memcpy(out, h.data() + off + (size_t)i * width, width); };
  std::vector<std::pair<unsigned long long, uint32_t>> order(n_out);  // (id, packed position)
  for (uint32_t i = 0; i < n_out; ++i) {
    at(pc * 16, 8, i, &order[i].first);
    order[i].second = i;
  }
  std::sort(order.begin(), order.end());
  for (uint32_t k = 0; k < n_out; ++k) {
    const uint32_t i = order[k].second;
    uint32_t r[4], state = 0;
    at(0, 16, i, r);
    at(pc * 36, 4, i, &state);
    if (out_task_id) out_task_id[k] = order[k].first;
    if (out_servant_idx) at(pc * 32, 4, i, &out_servant_idx[k]);
    if (out_expires_at) at(pc * 24, 8, i, &out_expires_at[k]);
    if (out_zombie) out_zombie[k] = (state & kLeaseZombie) ? 1 : 0;
    if (out_started_at) out_started_at[k] = (int64_t)((uint64_t)r[0] | ((uint64_t)r[1] << 32));
    if (out_env_id) out_env_id[k] = r[2];
    if (out_requestor_ip) out_requestor_ip[k] = r[3];
    if (out_prefetch) out_prefetch[k] = h[pc * 40 + i];
  }
  *out_n = n_out;
  *out_matches = matches;
  return YDC_OK;
}

int ydc_stream_inspect_count(ydc_context* c, const ydc_lease_filter* f, uint32_t n, uint32_t* out_matches) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (n > kSelectMaxFilters)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_count: %u filters > %u in one call", n, kSelectMaxFilters);
  if (n && (!f || !out_matches))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_inspect_count: %u filters without their columns", n);
  if (int rc = select_enter(c, "ydc_stream_inspect_count", f, n, 0)) return rc;
  if (!n) return YDC_OK;
  auto& sm = c->stream_mode;
  uint8_t* const d = sm.select.p;
  SelectState* const st = (SelectState*)d;
  YDC_LAUNCH(c, "k_select_count", k_select_count<false>, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, c->stream,
             sm.lt, sm.inspect.on ? sm.d_insp_rec.p : nullptr, sm.inspect.on ? sm.d_insp_pre.p : nullptr,
             (const LeaseFilter*)(d + kSelectFiltersAt), n, st);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint32_t got[kSelectMaxFilters];
  HIP_TRY(c, hipMemcpy(got, st->matches, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i)
    if (got[i] > sm.n_leases)
      return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u matches, |L| %u on the host", got[i], sm.n_leases);
  std::memcpy(out_matches, got, (size_t)n * 4);
  return YDC_OK;
}

// ---- the load per requestor (requestor_index.h) ----

// |L| + |W| as the index counts them in: L only where its records say whose a lease is.
static uint64_t requestor_entries(const ydc_context::Stream& sm) {
  return (uint64_t)(sm.leased() && sm.inspect.on ? sm.n_leases : 0u) + (uint64_t)(sm.waiting() ? sm.n_waiting : 0u);
}

// What both read calls of the requestor index do behind outlook_enter: the index over L and W as
// they are now, enqueued on the stream (the caller's kernel follows it there). *with_l: the lease
// columns are known.
static int requestor_index_build(ydc_context* c, RequestorIndex* out_ix, bool* with_l) {
  auto& sm = c->stream_mode;
  const bool with_w = sm.waiting();
  *with_l = sm.leased() && sm.inspect.on;
  const uint32_t slots = requestor_index_slots(requestor_entries(sm));
  const size_t o_sum = (size_t)slots * 8, o_un = o_sum + (size_t)slots * 4 * kRequestorCols;
  HIP_TRY(c, sm.requestor.d.reserve(o_un + 16));
  uint8_t* const b = sm.requestor.d.p;
  const RequestorIndex ix{(unsigned long long*)b, (uint32_t*)(b + o_sum), (uint32_t*)(b + o_un), slots - 1};
  *out_ix = ix;
  HIP_TRY(c, hipMemsetAsync(b, 0, o_un + 16, c->stream));  // every slot free, every sum 0
  const uint32_t combine = c->opt_requestor_combine ? 1u : 0u;
  if (*with_l && sm.n_leases)
    YDC_LAUNCH(c, "k_requestor_leases", k_requestor_leases, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0,
               c->stream, sm.lt, sm.d_insp_rec.p, sm.d_insp_pre.p, ix, combine);
  if (with_w && sm.n_waiting)
    YDC_LAUNCH(c, "k_requestor_waiting", k_requestor_waiting, dim3(ceil_div(sm.n_waiting, 256)), dim3(256), 0, c->stream,
               sm.wq.ip, sm.rw.n_imm, sm.rw.n_pre, sm.ws, sm.caps.max_waiting, ix, combine);
  HIP_TRY(c, hipGetLastError());
  return YDC_OK;
}

int ydc_stream_requestor_find(ydc_context* c, const uint32_t* requestor_ip, uint32_t n, ydc_requestor_load* out,
                              uint32_t* out_unattributed) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (n > (1u << 24))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_requestor_find: %u queries > 2^24 in one call", n);
  if (n && (!requestor_ip || !out))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_requestor_find: %u queries without their columns", n);
  static_assert(sizeof(ydc_requestor_load) == sizeof(RequestorLoad), "ydc_requestor_load");
  if (int rc = outlook_enter(c, "ydc_stream_requestor_find")) return rc;
  if (!n && !out_unattributed) return YDC_OK;
  auto& sm = c->stream_mode;
  RequestorIndex ix{};
  bool with_l = false;
  if (n) {  // (before the build is enqueued: a failed allocation leaves nothing in flight)
    HIP_TRY(c, sm.requestor.q.reserve(n));
    HIP_TRY(c, sm.requestor.res.reserve(n));
  }
  if (int rc = requestor_index_build(c, &ix, &with_l)) return rc;
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(sm.requestor.q.p, requestor_ip, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    YDC_LAUNCH(c, "k_requestor_find", k_requestor_find, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, sm.requestor.q.p,
               n, ix, with_l ? 1u : 0u, sm.requestor.res.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n) HIP_TRY(c, hipMemcpy(out, sm.requestor.res.p, (size_t)n * sizeof(RequestorLoad), hipMemcpyDeviceToHost));
  if (out_unattributed) {
    *out_unattributed = YDC_REQUESTOR_UNKNOWN;
    if (with_l) HIP_TRY(c, hipMemcpy(out_unattributed, ix.unattributed, 4, hipMemcpyDeviceToHost));
  }
  return YDC_OK;
}

int ydc_stream_requestor_get(ydc_context* c, ydc_requestor_load* out, uint32_t cap, uint32_t* out_n,
                             uint32_t* out_unattributed) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  *out_n = 0;
  if (int rc = outlook_enter(c, "ydc_stream_requestor_get")) return rc;
  auto& sm = c->stream_mode;
  RequestorIndex ix{};
  bool with_l = false;
  // The fold's ticket, count and look-back words | its rows: a requestor has at least one entry.
  const uint64_t most = requestor_entries(sm);
  const uint32_t slots = requestor_index_slots(most), tiles = ceil_div(slots, kRequestorTile);
  const uint32_t room = (uint32_t)std::min<uint64_t>(most, slots);
  size_t off = 0;
  const size_t o_state = section(&off, sizeof(RequestorFoldState)), o_lb = section(&off, (size_t)tiles * 8);
  const size_t clear = off;
  const size_t o_rows = section(&off, (size_t)room * sizeof(RequestorLoad));
  HIP_TRY(c, sm.requestor.rows.reserve(off));
  if (int rc = requestor_index_build(c, &ix, &with_l)) return rc;
  uint8_t* const b = sm.requestor.rows.p;
  RequestorFoldState* const fs = (RequestorFoldState*)(b + o_state);
  RequestorLoad* const rows = (RequestorLoad*)(b + o_rows);
  uint32_t m = 0;
  if (most) {
    HIP_TRY(c, hipMemsetAsync(b, 0, clear, c->stream));
    YDC_LAUNCH(c, "k_requestor_fold", k_requestor_fold, dim3(tiles), dim3(256), 0, c->stream, ix, with_l ? 1u : 0u, fs,
               (unsigned long long*)(b + o_lb), rows, room);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (most) HIP_TRY(c, hipMemcpy(&m, &fs->n_rows, 4, hipMemcpyDeviceToHost));
  if (m > room) return fail(c, YDC_ERR_NOT_CONVERGED, "%u requestors among %u entries", m, room);
  *out_n = m;
  if (m > cap) return fail(c, YDC_ERR_CAPACITY, "%u requestors > cap %u", m, cap);
  if (m && !out) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_requestor_get: %u rows without their column", m);
  if (m) HIP_TRY(c, hipMemcpy(out, rows, (size_t)m * sizeof(RequestorLoad), hipMemcpyDeviceToHost));
  if (out_unattributed) {
    *out_unattributed = YDC_REQUESTOR_UNKNOWN;
    if (with_l) HIP_TRY(c, hipMemcpy(out_unattributed, ix.unattributed, 4, hipMemcpyDeviceToHost));
  }
  return YDC_OK;
}

int ydc_admit_clip(const uint32_t* requestor_ip, const uint32_t* n_immediate, const uint32_t* n_prefetch, uint32_t n,
                   const ydc_requestor_load* load, uint32_t cap, uint32_t* out_immediate, uint32_t* out_prefetch) {
  static_assert(sizeof(ydc_requestor_load) == sizeof(AdmitLoad), "ydc_requestor_load");
  if (!n) return YDC_OK;
  if (!requestor_ip || !n_immediate || !load || !out_immediate || (n_prefetch && !out_prefetch))
    return YDC_ERR_INVALID_ARGUMENT;
  return admit_clip(requestor_ip, n_immediate, n_prefetch, n, reinterpret_cast<const AdmitLoad*>(load), cap,
                    out_immediate, out_prefetch)
             ? YDC_OK
             : YDC_ERR_INVALID_ARGUMENT;
}

int ydc_stream_waiting_take(ydc_context* c, uint64_t* out_tags, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n || !c->stream_mode.active || !c->stream_mode.waiting()) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpy(&n, &sm.ws->count, 4, hipMemcpyDeviceToHost));
  *out_n = n;
  if (n > cap) return fail(c, YDC_ERR_CAPACITY, "%u waiting requests > cap %u", n, cap);
  if (n && !out_tags) return YDC_ERR_INVALID_ARGUMENT;
  if (n) HIP_TRY(c, hipMemcpy(out_tags, sm.wq.tag, (size_t)n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemsetAsync(&sm.ws->count, 0, 4, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  sm.n_waiting = sm.n_wait_rows = 0;
  return YDC_OK;
}

int ydc_stream_buffers_get(ydc_context* c, ydc_stream_buffers* out) {
  if (!c || !out || !c->stream_mode.active) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  out->upd_idx = sm.h.upd_idx;
  out->upd_rows = sm.h.upd_rows;
  out->release_servant_idx = sm.h.rel;
  out->env_id = sm.h.env;
  out->min_version = sm.h.minv;
  out->requestor_ip = sm.h.ip;
  out->out_servant_idx = sm.h_out;
  return YDC_OK;
}

int ydc_stream_end(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  join_lanes(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stream_release(c);
  return YDC_OK;
}

int ydc_stream_tick(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                    uint32_t n_upd, const uint32_t* release_servant_idx, uint32_t n_rel,
                    const ydc_task_soa* tasks, uint32_t n_tasks, uint32_t* out_servant_idx) {
  return ydc_stream_tick_wide(c, upd_idx, upd_rows, nullptr, 1, n_upd, release_servant_idx, n_rel, tasks,
                              n_tasks, out_servant_idx);
}

// Waiting mode, after the step: the resolved list to the caller, the host's mirror of |W| and the
// statistics (padding — W's unused or expired slots, the new region's tail — counts nowhere).
static int stream_wait_finish(ydc_context* c, const WaitTick* wt, uint32_t n_tasks) {
  auto& sm = c->stream_mode;
  const uint32_t n_res = std::min(sm.h_wout->n_resolved, sm.caps.max_waiting);
  const uint32_t n_wait = sm.h_wout->n_waiting;
  if (n_wait > sm.caps.max_waiting)
    return fail(c, YDC_ERR_NOT_CONVERGED, "waiting queue of %u > max_waiting %u", n_wait, sm.caps.max_waiting);
  uint32_t expired = 0;  // (a resolved Timeout is an expired entry: a live one that timed out stays)
  for (uint32_t i = 0; i < n_res; ++i)  // (a withdrawn entry was placed as an expired one)
    expired += sm.h_res_idx[i] == YDC_IDX_TIMEOUT || sm.h_res_idx[i] == YDC_IDX_WITHDRAWN;
  if (n_res && wt->out_resolved_tags != sm.h_res_tag)
    std::memcpy(wt->out_resolved_tags, sm.h_res_tag, (size_t)n_res * 8);
  if (n_res && wt->out_resolved_idx != sm.h_res_idx)
    std::memcpy(wt->out_resolved_idx, sm.h_res_idx, (size_t)n_res * 4);
  if (n_res && wt->out_resolved_task_id) std::memcpy(wt->out_resolved_task_id, sm.h_res_id, (size_t)n_res * 8);
  *wt->out_n_resolved = n_res;
  *wt->out_n_waiting = n_wait;
  const uint32_t live = sm.n_waiting - std::min(sm.n_waiting, expired);
  c->stats.n_tasks = n_tasks + live;
  // (the new region's padding is taken off by the caller, as in a plain tick; W's here)
  c->stats.env_not_found -= std::min(c->stats.env_not_found, sm.caps.max_waiting - live);
  sm.n_waiting = n_wait;
  sm.last_now = wt->now;
  return YDC_OK;
}

// The lease outcome block is this tick's and |L| is in range.
static bool stream_lease_outcome_ok(const ydc_context::Stream& sm) {
  if (sm.max_book && (sm.book.h_bout->tick_no != sm.lease_tick || sm.book.h_bout->n_entries > sm.max_book)) return false;
  return sm.h_lout->tick_no == sm.lease_tick && sm.h_lout->n_leases <= sm.caps.max_leases;
}

// What the steps of a tick hand on to the steps behind them (stream_tick). Leaving a tick while
// the removal route's leases are parked, by whichever return, sweeps them.
struct TickState {
  ydc_context* c;
  uint32_t rows_new = 0;    // check: the rows of an rpc tick's new requests
  uint32_t n_ids = 0;       // check: the reported ids
  bool structural = false;  // heartbeats: they took the eager path
  uint32_t graph_upd = 0;   // heartbeats, expiry: the heartbeats that are left to the step
  bool parked = false;      // expiry: the tick removes servants, and their leases are parked
  LeaseTick lt_alive{};     // expiry: the lease arguments with the reports renumbered
  BatchPlan eager;          // run: the plan of a batch the host placed itself
  const BatchPlan* plan = nullptr;  // run: the plan the batch was placed with
  uint32_t rounds = 0;              // run: ... and the passes it took
  ~TickState() {
    if (parked) alive_orphans_after_error(c);
  }
};

// The lease part of a tick's ending, once the outcome is known to be good: renewal and report
// answers to the caller, the host's mirror of |L| and the statistics. n_ids: the reported ids.
static void stream_lease_apply(ydc_context* c, const LeaseTick* lt, uint32_t n_ids) {
  auto& sm = c->stream_mode;
  const LeaseOutcome& o = *sm.h_lout;
  if (lt->n_renew) std::memcpy(lt->out_renewed, sm.h_renewed, lt->n_renew);
  if (n_ids) std::memcpy(lt->out_unknown, sm.h_unknown, n_ids);
  *lt->out_n_leases = o.n_leases;
  c->stats.leases_expired = o.expired;
  c->stats.leases_swept = o.swept;
  c->stats.leases_freed = o.freed;
  c->stats.renewals_refused = o.renew_refused;
  sm.n_leases = o.n_leases;
  if (sm.max_book) sm.book.n = sm.book.h_bout->n_entries;
  sm.last_now = lt->now;
}

// Leased mode, after the step: the ids and the lease part.
static int stream_lease_finish(ydc_context* c, const LeaseTick* lt, uint32_t n_tasks, uint32_t n_ids) {
  auto& sm = c->stream_mode;
  if (!stream_lease_outcome_ok(sm))
    return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: outcome of tick %u (expected %u), %u leases of %u",
                sm.h_lout->tick_no, sm.lease_tick, sm.h_lout->n_leases, sm.caps.max_leases);
  stream_lease_apply(c, lt, n_ids);
  if (n_tasks) std::memcpy(lt->out_task_id, sm.h_task_id, (size_t)n_tasks * 8);
  return YDC_OK;
}

// RPC mode, after the step: every list to the caller, the host's mirrors of |W|, rows(W) and |L|,
// and the statistics (n_tasks counts the batch's rows; padding counts nowhere).
static int stream_rpc_finish(ydc_context* c, const StreamCall& t, const TickState& ts) {
  auto& sm = c->stream_mode;
  const WaitTick* wt = t.wt;
  const LeaseTick* lt = t.lt;
  const RpcTick* rt = t.rt;
  const LeaseOutcome& lo = *sm.h_lout;
  const RpcOutcome& o = *sm.rh.outcome;
  if (!stream_lease_outcome_ok(sm) || o.n_waiting > sm.caps.max_waiting || o.n_resolved > sm.caps.max_waiting ||
      o.n_rows > sm.caps.max_rows || o.n_res_grants > sm.caps.max_rows)
    return fail(c, YDC_ERR_NOT_CONVERGED, "rpc stream: outcome of tick %u (expected %u), %u leases, %u waiting, %u rows",
                lo.tick_no, sm.lease_tick, lo.n_leases, o.n_waiting, o.n_rows);
  if (ts.rows_new) {
    std::memcpy(t.out_servant_idx, sm.rh.new_srv, (size_t)ts.rows_new * 4);
    std::memcpy(lt->out_task_id, sm.rh.new_id, (size_t)ts.rows_new * 8);
  }
  if (t.n_tasks) {
    std::memcpy(rt->out_status, sm.rh.status, (size_t)t.n_tasks * 4);
    std::memcpy(rt->out_n_granted, sm.rh.n_granted, (size_t)t.n_tasks * 4);
  }
  if (o.n_resolved) {
    std::memcpy(wt->out_resolved_tags, sm.rh.res_tag, (size_t)o.n_resolved * 8);
    std::memcpy(wt->out_resolved_idx, sm.rh.res_status, (size_t)o.n_resolved * 4);
    std::memcpy(rt->out_resolved_n_granted, sm.rh.res_n, (size_t)o.n_resolved * 4);
    std::memcpy(rt->out_resolved_first, sm.rh.res_first, (size_t)o.n_resolved * 4);
  }
  if (o.n_res_grants) {
    std::memcpy(rt->out_resolved_servant_idx, sm.rh.res_srv, (size_t)o.n_res_grants * 4);
    std::memcpy(wt->out_resolved_task_id, sm.rh.res_id, (size_t)o.n_res_grants * 8);
  }
  stream_lease_apply(c, lt, ts.n_ids);
  *wt->out_n_resolved = o.n_resolved;
  *wt->out_n_waiting = o.n_waiting;
  *rt->out_n_waiting_rows = o.n_waiting_rows;
  c->stats.n_tasks = o.n_rows;
  c->stats.env_not_found -= std::min(c->stats.env_not_found, sm.caps.max_rows - o.n_rows);  // padding
  sm.n_waiting = o.n_waiting;
  sm.n_wait_rows = o.n_waiting_rows;
  return YDC_OK;
}

// After a placement the host ran itself: the answers into the page-locked result array — in
// waiting mode by k_wait_compact, in leased mode by k_lease_grant, with both by
// k_wait_lease_commit (ungated), otherwise by a copy. `a`: the arena where the step
// read the tick's clock. That is the device mirror (d) when the tick copied the arena there, and
// the page-locked arena in place (z) when it did not: the mirror then still holds an older
// tick's clock.
static int stream_answer_eager(ydc_context* c, const TickArena& a) {
  auto& sm = c->stream_mode;
  if (sm.waiting() || sm.leased()) {  // (ungated; in leased mode with the ids and the leases)
    enqueue_stream_answer(c, a, nullptr, kNone);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
  } else {
    HIP_TRY(c, hipMemcpy(sm.h_out, c->d_out_idx.p, (size_t)sm.caps.max_tasks * 4, hipMemcpyDeviceToHost));
  }
  return YDC_OK;
}

// ---- a tick, step by step: check, heartbeats, servants' expiry, stage, run, finish ----

// Step 1: everything a tick can be refused for, in a fixed order, before anything of the stream
// or the registry is written — except the stamps of the two OnceMarks, which a refused tick may
// leave advanced. Hands on: the rows of an rpc tick's new requests and the reported ids.
static int stream_tick_check(ydc_context* c, const StreamCall& t, TickState* ts) {
  auto& sm = c->stream_mode;
  const WaitTick* wt = t.wt;
  const LeaseTick* lt = t.lt;
  const RpcTick* rt = t.rt;
  const uint32_t n_upd = t.n_upd, n_tasks = t.n_tasks;
  // A stream takes the ticks of its mode. Of the stream's mode and the call's, the one that has
  // more parts names the mismatch.
  static const struct {
    const char *begin, *tick, *part;
  } kModes[] = {{"ydc_stream_begin", "ydc_stream_tick", ""},
                {"ydc_stream_begin_waiting", "ydc_stream_tick_waiting", "a waiting queue"},
                {"ydc_stream_begin_leased", "ydc_stream_tick_leased", "a lease table"},
                {"ydc_stream_begin_waiting_leased", "ydc_stream_tick_waiting_leased", "a waiting queue and a lease table"},
                {"ydc_stream_begin_rpc", "ydc_stream_tick_rpc", "ydc_stream_begin_rpc"}};
  const int has = sm.rpc() ? 4 : sm.waiting() && sm.leased() ? 3 : sm.leased() ? 2 : sm.waiting() ? 1 : 0;
  const int got = rt ? 4 : wt && lt ? 3 : lt ? 2 : wt ? 1 : 0;
  if (has > got)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "a context begun with %s takes %s", kModes[has].begin, kModes[has].tick);
  if (got > has)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s on a context begun without %s", kModes[got].tick, kModes[got].part);
  if (n_upd > sm.caps.max_updates || t.n_rel > sm.caps.max_releases || n_tasks > sm.caps.max_tasks)
    return fail(c, YDC_ERR_CAPACITY, "tick (%u updates, %u releases, %u tasks) exceeds the capacity "
                "given to ydc_stream_begin (%u, %u, %u)", n_upd, t.n_rel, n_tasks, sm.caps.max_updates,
                sm.caps.max_releases, sm.caps.max_tasks);
  if ((n_upd && (!t.upd_idx || !t.upd_rows)) || (t.n_rel && !t.rel) || (n_tasks && (!t.tasks || !t.out_servant_idx)))
    return YDC_ERR_INVALID_ARGUMENT;
  // (one clock per tick: a waiting tick meets this refusal in its own part, a leased one in its)
  const int64_t now = wt ? wt->now : lt ? lt->now : 0;
  auto clock_runs_back = [&] {
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "now %lld is before the previous tick's %lld", (long long)now,
                (long long)sm.last_now);
  };
  if (wt) {
    // (nothing is applied unless the whole tick is acceptable)
    if ((uint64_t)sm.n_waiting + n_tasks > sm.caps.max_waiting)
      return fail(c, YDC_ERR_CAPACITY, "%u waiting + %u new requests > max_waiting %u", sm.n_waiting, n_tasks,
                  sm.caps.max_waiting);
    if (now < sm.last_now) return clock_runs_back();
    if ((n_tasks && (!wt->deadlines || !wt->tags)) || !wt->out_n_resolved || !wt->out_n_waiting ||
        !wt->out_resolved_tags || !wt->out_resolved_idx || (lt && !wt->out_resolved_task_id))
      return YDC_ERR_INVALID_ARGUMENT;
  }
  if (lt) {
    // (nothing is applied unless the whole tick is acceptable)
    if (lt->n_renew > sm.caps.max_renewals || lt->n_free > sm.caps.max_frees || lt->n_rep > sm.caps.max_reports)
      return fail(c, YDC_ERR_CAPACITY, "tick (%u renewals, %u frees by id, %u reports) exceeds the capacity given "
                  "to ydc_stream_begin_leased (%u, %u, %u)", lt->n_renew, lt->n_free, lt->n_rep, sm.caps.max_renewals,
                  sm.caps.max_frees, sm.caps.max_reports);
    if ((lt->n_renew && (!lt->renew_id || !lt->renew_exp || !lt->out_renewed)) || (lt->n_free && !lt->free_id) ||
        (lt->n_rep && (!lt->rep_srv || !lt->rep_off)) || (n_tasks && (!lt->lease_exp || !lt->out_task_id)) ||
        !lt->out_n_leases)
      return YDC_ERR_INVALID_ARGUMENT;
    // (with a waiting queue: every waiting entry may be granted in this tick)
    if (!rt && wt && (uint64_t)sm.n_leases + sm.n_waiting + n_tasks > sm.caps.max_leases)
      return fail(c, YDC_ERR_CAPACITY, "%u leases + %u waiting + %u new requests > max_leases %u", sm.n_leases,
                  sm.n_waiting, n_tasks, sm.caps.max_leases);
    if (!rt && (uint64_t)sm.n_leases + n_tasks > sm.caps.max_leases)
      return fail(c, YDC_ERR_CAPACITY, "%u leases + %u new requests > max_leases %u", sm.n_leases, n_tasks,
                  sm.caps.max_leases);
    if (rt) {
      // (every row of W's entries and of the new requests may be granted in this tick)
      if ((n_tasks && (!rt->n_imm || !rt->n_pre || !rt->out_status || !rt->out_n_granted)) ||
          !rt->out_resolved_n_granted || !rt->out_resolved_first || !rt->out_resolved_servant_idx ||
          !rt->out_n_waiting_rows)
        return YDC_ERR_INVALID_ARGUMENT;
      uint64_t rows = 0;
      for (uint32_t i = 0; i < n_tasks; ++i) {
        const uint64_t r = (uint64_t)rt->n_imm[i] + rt->n_pre[i];
        if (!r) return fail(c, YDC_ERR_INVALID_ARGUMENT, "request %u asks for no grant (n_immediate + n_prefetch == 0)", i);
        rows += r;
      }
      if (sm.n_wait_rows + rows > sm.caps.max_rows)
        return fail(c, YDC_ERR_CAPACITY, "%u waiting rows + %llu new rows > max_rows %u", sm.n_wait_rows,
                    (unsigned long long)rows, sm.caps.max_rows);
      if ((uint64_t)sm.n_leases + sm.n_wait_rows + rows > sm.caps.max_leases)
        return fail(c, YDC_ERR_CAPACITY, "%u leases + %u waiting rows + %llu new rows > max_leases %u", sm.n_leases,
                    sm.n_wait_rows, (unsigned long long)rows, sm.caps.max_leases);
      ts->rows_new = (uint32_t)rows;
    }
    if (!wt && now < sm.last_now) return clock_runs_back();
    if (lt->n_rep) {
      if (lt->rep_off[0] != 0) return fail(c, YDC_ERR_INVALID_ARGUMENT, "report_off[0] must be 0");
      for (uint32_t r = 0; r < lt->n_rep; ++r)
        if (lt->rep_off[r + 1] < lt->rep_off[r])
          return fail(c, YDC_ERR_INVALID_ARGUMENT, "report_off must not decrease (entry %u)", r + 1);
      const uint32_t n_ids = lt->rep_off[lt->n_rep];
      if (n_ids > sm.caps.max_report_ids)
        return fail(c, YDC_ERR_CAPACITY, "%u reported ids > max_report_ids %u", n_ids, sm.caps.max_report_ids);
      if (n_ids && (!lt->rep_id || !lt->out_unknown)) return YDC_ERR_INVALID_ARGUMENT;
      ts->n_ids = n_ids;
      // A servant reports at most once per tick (a servant this tick's heartbeats add may report too).
      uint32_t S = c->reg.n;
      for (uint32_t i = 0; i < n_upd; ++i) S = std::max(S, t.upd_idx[i] + 1);
      sm.rep_once.begin(S);
      for (uint32_t r = 0; r < lt->n_rep; ++r) {
        const uint32_t s = lt->rep_srv[r];
        if (s >= S || !sm.rep_once.first(s))
          return fail(c, YDC_ERR_INVALID_ARGUMENT, "report %u names servant %u, which is unknown or reports twice", r, s);
      }
    }
    if (sm.max_book) {
      // (conservative like the |L| bound: every reported id may be permitted, no entry dropped)
      if (sm.book.staged.on && sm.book.staged.stid.size() != ts->n_ids)
        return fail(c, YDC_ERR_INVALID_ARGUMENT, "%zu ids staged with ydc_stream_book_stage, %u reported",
                    sm.book.staged.stid.size(), ts->n_ids);
      if ((uint64_t)sm.book.n + ts->n_ids > sm.max_book)
        return fail(c, YDC_ERR_CAPACITY, "%u book entries + %u reported ids > max_book %u", sm.book.n, ts->n_ids,
                    sm.max_book);
    }
  }
  if (sm.alive.on) {
    // Every heartbeat brings its expiry, and a servant at most one (k_apply_tick leaves the winner of
    // two rows for one servant undefined; an expiry cannot be).
    if (sm.alive.staged ? sm.alive.stage.size() != n_upd : n_upd != 0)
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "%u heartbeats, %zu expiries staged with ydc_stream_alive_stage", n_upd,
                  sm.alive.staged ? sm.alive.stage.size() : (size_t)0);
    const uint64_t S = (uint64_t)c->reg.n + n_upd;  // (the tick's heartbeats may add that many rows)
    sm.alive.once.begin(S);
    for (uint32_t i = 0; i < n_upd; ++i) {
      const uint32_t s = t.upd_idx[i];
      if (s >= S) return fail(c, YDC_ERR_INVALID_ARGUMENT, "servant index %u out of order", s);
      if (!sm.alive.once.first(s))
        return fail(c, YDC_ERR_INVALID_ARGUMENT, "heartbeat %u names servant %u a second time", i, s);
    }
  }
  if (t.upd_env_masks && (t.env_words == 0 || t.env_words > YDC_MAX_ENV_WORDS))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "env_words %u out of range", t.env_words);
  // Without masks (the plain form), rows of a table with several mask words cannot say what the
  // servant advertises: a known servant keeps its environments, and a NEW one (which would
  // silently have none) is refused.
  if (!t.upd_env_masks && c->reg.env_words > 1)
    for (uint32_t i = 0; i < n_upd; ++i)
      if (t.upd_idx[i] >= c->reg.n)
        return fail(c, YDC_ERR_INVALID_ARGUMENT, "a tick that adds a servant to a table with %u mask "
                    "words needs its environments: use ydc_stream_tick_wide", c->reg.env_words);
  return YDC_OK;
}

// All of a tick's heartbeats applied to the registry now, the way a structural one has to go.
static int stream_heartbeats_eager(ydc_context* c, const StreamCall& t) {
  const uint32_t EW = c->reg.env_words, n_upd = t.n_upd;
  if (t.upd_env_masks) return ydc_update_servants_wide(c, t.upd_idx, t.upd_rows, t.upd_env_masks, t.env_words, n_upd);
  if (EW == 1) return ydc_update_servants(c, t.upd_idx, t.upd_rows, n_upd);
  // Rows without masks on a wide table: the (known) servants keep their environments.
  std::vector<uint64_t> env((size_t)n_upd * EW, 0);
  for (uint32_t i = 0; i < n_upd; ++i)
    if (t.upd_idx[i] < c->reg.n)  // (new servants were refused by the check)
      std::copy_n(&c->reg.env[(size_t)t.upd_idx[i] * EW], EW, &env[(size_t)i * EW]);
  return ydc_update_servants_wide(c, t.upd_idx, t.upd_rows, env.data(), EW, n_upd);
}

// Step 2, the heartbeats: structural ones (and new servants) take the eager path — with masks (the
// wide form) a changed environment set is structural like any other change — and leave nothing
// to the step; the others are mirrored on the host and left to k_apply_tick.
static int stream_tick_heartbeats(ydc_context* c, const StreamCall& t, TickState* ts) {
  auto& sm = c->stream_mode;
  for (uint32_t i = 0; i < t.n_upd && !ts->structural; ++i)
    ts->structural = c->reg.structural(t.upd_idx[i], t.upd_rows[i], t.upd_env_masks, t.env_words, i);
  ts->graph_upd = t.n_upd;
  if (ts->structural) {
    if (int rc = stream_heartbeats_eager(c, t)) return rc;
    ts->graph_upd = 0;
  } else {
    for (uint32_t i = 0; i < t.n_upd; ++i) c->reg.store_light(t.upd_idx[i], t.upd_rows[i]);
  }
  // Inspection (stream_inspect.h): a servant this tick's heartbeats appended was discovered now.
  if (sm.inspect.on)
    if (int rc = inspect_fit(c, t.lt->now)) return rc;
  return YDC_OK;
}

// Step 3, aliveness (servant_alive.h): the whole of OnExpirationTimer. No servant can be due while the
// host's bound of min(E) is not below the clock; when it is, k_alive_due says who is, and a tick in
// which somebody is takes the removal route here, in front of the step: the due rows leave the registry,
// their leases are parked, and `t` gets the releases and reports rewritten in the new numbering.
static int stream_tick_expiry(ydc_context* c, StreamCall& t, TickState* ts) {
  auto& sm = c->stream_mode;
  auto& al = sm.alive;
  const int64_t now = t.lt->now;
  const uint32_t n_upd = t.n_upd;
  if (int rc = alive_fit(c)) return rc;  // (rows the heartbeats added: "never" until filed below)
  const int64_t* stage = al.stage.data();
  for (uint32_t i = 0; i < n_upd; ++i) al.bound = std::min(al.bound, stage[i]);
  const bool alarm = al.bound < now;
  // Heartbeats that took the eager path: so do their expiries. In front of an alarm the others' are
  // filed as well (and again inside the step: idempotent).
  if (ts->structural || alarm)
    if (int rc = alive_file(c, t.upd_idx, stage, n_upd)) return rc;
  al.removed.clear();
  al.orphans = 0;
  uint32_t n_due = 0;
  if (alarm)
    if (int rc = alive_due(c, now, &n_due)) return rc;
  if (!n_due) return YDC_OK;
  if (!ts->structural) {  // (all of the tick's heartbeats eagerly, as the structural branch does)
    if (int rc = stream_heartbeats_eager(c, t)) return rc;
    ts->graph_upd = 0;
  }
  const uint32_t* due = (const uint32_t*)al.due.p;
  al.removed.assign(due, due + n_due);
  const uint32_t* gone = al.removed.data();
  ts->parked = true;
  if (int rc = remove_rows(c, gone, n_due, true)) return rc;
  al.removals += n_due;
  // The staged tick in the new numbering (the reports were validated on the caller's, by the check).
  al.rel.assign(t.rel, t.rel + t.n_rel);
  for (uint32_t& s : al.rel) s = alive_renumber(gone, n_due, s);
  t.rel = al.rel.data();
  al.rep.assign(t.lt->rep_srv, t.lt->rep_srv + t.lt->n_rep);
  for (uint32_t& s : al.rep) s = alive_renumber(gone, n_due, s);
  ts->lt_alive = *t.lt;
  ts->lt_alive.rep_srv = al.rep.data();
  t.lt = &ts->lt_alive;
  return YDC_OK;
}

// ---- usage per requestor (stream_usage.h) ----

static size_t usage_table_bytes(uint32_t slots) { return (size_t)slots * 8 * (1 + kUsageCols); }

// The table over a buffer of `slots` slots: word | the five sums.
static UsageTable usage_table_at(uint8_t* b, uint32_t slots, UsageState* st) {
  return UsageTable{(unsigned long long*)b, (unsigned long long*)(b + (size_t)slots * 8), st, slots - 1};
}

// What the next accrual can meet in L and W that the table may not hold yet, when nothing narrower is known.
static uint64_t usage_holders(const ydc_context::Stream& sm) {
  return (uint64_t)sm.n_leases + (sm.waiting() ? sm.n_waiting : 0u);
}

// The bound that errs high on the distinct keys the table can hold after the next accrual: the keys it
// has, plus those L and W can have gained since they were last claimed, which are no more than L and W hold.
static uint64_t usage_bound(const ydc_context::Stream& sm) {
  return (uint64_t)sm.usage.n_keys + std::min<uint64_t>(sm.usage.fresh, usage_holders(sm));
}

// Room for `keys` distinct requestors at a load of 1/2 at the most. A table that has to grow is filed
// again into a larger one (k_usage_rehash), all or nothing, and the step is captured again: it holds
// the table's addresses. The stream is brought to rest first.
static int usage_fit(ydc_context* c, uint64_t keys) {
  auto& sm = c->stream_mode;
  auto& u = sm.usage;
  const uint32_t want = usage_slots(keys);
  if (want <= u.slots()) return YDC_OK;
  if (2 * keys > want) return fail(c, YDC_ERR_CAPACITY, "usage: %llu requestors > 2^30", (unsigned long long)keys);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevBuf<uint8_t> bigger;
  HIP_TRY(c, bigger.reserve(usage_table_bytes(want)));
  HIP_TRY(c, hipMemsetAsync(bigger.p, 0, usage_table_bytes(want), c->stream));
  HIP_TRY(c, hipMemsetAsync(&u.st.p->n_keys, 0, 4, c->stream));  // (the claims count the keys again)
  const UsageTable grown = usage_table_at(bigger.p, want, u.st.p);
  YDC_LAUNCH(c, "k_usage_rehash", k_usage_rehash, dim3(ceil_div(u.slots(), 256)), dim3(256), 0, c->stream, u.tb, grown);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  UsageState s{};
  HIP_TRY(c, hipMemcpy(&s, u.st.p, sizeof s, hipMemcpyDeviceToHost));
  if (s.n_keys != u.n_keys || s.dropped)
    return fail(c, YDC_ERR_NOT_CONVERGED, "usage: %u of %u requestors filed again (%u dropped)", s.n_keys, u.n_keys, s.dropped);
  u.d = std::move(bigger);
  u.tb = grown;
  sm.stale = true;
  return YDC_OK;
}

static int usage_enter(ydc_context* c, const char* who) {
  const auto& sm = c->stream_mode;
  if (!sm.active || !sm.usage.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the stream keeps no usage (ydc_stream_usage_begin)", who);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return YDC_OK;
}

int ydc_stream_usage_begin(ydc_context* c, int64_t quantum, uint32_t want_requestors) {
  if (!c || quantum <= 0) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active || !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_begin: no leased, waiting-and-leased or rpc stream is open");
  if (!sm.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_begin: inspection is off, so no lease says whose it is "
                "(ydc_stream_inspect_begin)");
  if (want_requestors > (1u << 30))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "want_requestors %u out of range (0 .. 2^30)", want_requestors);
  HIP_TRY(c, hipSetDevice(c->device));
  auto& u = sm.usage;
  if (u.on) {
    if (quantum != u.quantum)
      return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_begin: quantum %lld, the capability is on with %lld",
                  (long long)quantum, (long long)u.quantum);
    return usage_fit(c, want_requestors);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ydc_context::Stream::Usage n;
  const uint32_t slots = usage_slots(want_requestors);
  HIP_TRY(c, n.d.reserve(usage_table_bytes(slots)));
  HIP_TRY(c, n.st.reserve(1));
  HIP_TRY(c, n.h.reserve(64 + sizeof(UsageDone)));
  HIP_TRY(c, hipMemset(n.d.p, 0, usage_table_bytes(slots)));
  HIP_TRY(c, hipMemset(n.st.p, 0, sizeof(UsageState)));
  std::memset(n.h.p, 0, 64 + sizeof(UsageDone));
  n.tb = usage_table_at(n.d.p, slots, n.st.p);
  n.h_dq = (unsigned long long*)n.h.p;
  n.z_dq = (unsigned long long*)n.h.z;
  n.h_done = (UsageDone*)(n.h.p + 64);
  n.z_done = (UsageDone*)(n.h.z + 64);
  n.quantum = quantum;
  // The clock at this call: the stream's last now; before its first tick, that tick's own.
  n.has_last = sm.last_now != INT64_MIN;
  n.last = n.has_last ? sm.last_now : 0;
  n.fresh = usage_holders(sm);
  n.on = true;
  u = std::move(n);
  sm.stale = true;  // (the step gains a launch)
  return YDC_OK;
}

int ydc_stream_usage_get(ydc_context* c, ydc_usage_row* rows, uint32_t cap, uint32_t* out_n, ydc_usage_totals* totals,
                         uint32_t flags) {
  if (!c || !out_n) return YDC_ERR_INVALID_ARGUMENT;
  static_assert(sizeof(ydc_usage_row) == sizeof(UsageRow), "ydc_usage_row");
  if (flags & ~YDC_USAGE_RESET) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_get: flags %#x", flags);
  if (int rc = usage_enter(c, "ydc_stream_usage_get")) return rc;
  auto& sm = c->stream_mode;
  auto& u = sm.usage;
  UsageState s{};
  HIP_TRY(c, hipMemcpy(&s, u.st.p, sizeof s, hipMemcpyDeviceToHost));
  const uint32_t m = s.n_keys;
  if (m > u.slots()) return fail(c, YDC_ERR_NOT_CONVERGED, "usage: %u requestors in %u slots", m, u.slots());
  if (m > cap) {
    *out_n = m;
    return fail(c, YDC_ERR_CAPACITY, "%u requestors > cap %u", m, cap);
  }
  if (m && !rows) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_get: %u rows without their column", m);
  if (m) {
    const uint32_t tiles = ceil_div(u.slots(), kUsageTile);
    size_t off = 0;
    const size_t o_state = section(&off, sizeof(UsageFoldState)), o_lb = section(&off, (size_t)tiles * 8);
    HIP_TRY(c, u.fold.reserve(off));
    HIP_TRY(c, u.rows.reserve(m));
    uint8_t* const b = u.fold.p;
    UsageFoldState* const fs = (UsageFoldState*)(b + o_state);
    HIP_TRY(c, hipMemsetAsync(b, 0, off, c->stream));
    YDC_LAUNCH(c, "k_usage_fold", k_usage_fold, dim3(tiles), dim3(256), 0, c->stream, u.tb, fs,
               (unsigned long long*)(b + o_lb), u.rows.p, m);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t got = 0;
    HIP_TRY(c, hipMemcpy(&got, &fs->n_rows, 4, hipMemcpyDeviceToHost));
    if (got != m) return fail(c, YDC_ERR_NOT_CONVERGED, "usage: %u rows folded, %u requestors", got, m);
    HIP_TRY(c, hipMemcpy(rows, u.rows.p, (size_t)m * sizeof(UsageRow), hipMemcpyDeviceToHost));
  }
  *out_n = m;
  if (totals) *totals = ydc_usage_totals{s.unattributed, s.quanta, s.ticks, m, u.slots()};
  if (flags & YDC_USAGE_RESET) {  // (keys included: the next accrual claims today's holders again)
    HIP_TRY(c, hipMemset(u.d.p, 0, usage_table_bytes(u.slots())));
    HIP_TRY(c, hipMemset(u.st.p, 0, sizeof(UsageState)));
    u.n_keys = 0;
    u.fresh = usage_holders(sm);
  }
  return YDC_OK;
}

int ydc_stream_usage_find(ydc_context* c, const uint32_t* requestor_ip, uint32_t n, ydc_usage_row* out) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (n > (1u << 24)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_find: %u queries > 2^24 in one call", n);
  if (n && (!requestor_ip || !out))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_find: %u queries without their columns", n);
  if (int rc = usage_enter(c, "ydc_stream_usage_find")) return rc;
  if (!n) return YDC_OK;
  auto& u = c->stream_mode.usage;
  HIP_TRY(c, u.q.reserve(n));
  HIP_TRY(c, u.rows.reserve(n));
  HIP_TRY(c, hipMemcpyAsync(u.q.p, requestor_ip, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  YDC_LAUNCH(c, "k_usage_find", k_usage_find, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, u.q.p, n, u.tb, u.rows.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, u.rows.p, (size_t)n * sizeof(UsageRow), hipMemcpyDeviceToHost));
  return YDC_OK;
}

int ydc_stream_usage_load(ydc_context* c, const ydc_usage_row* rows, uint32_t n, const ydc_usage_totals* add) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (n > (1u << 24)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_load: %u rows > 2^24 in one call", n);
  if (n && !rows) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_usage_load: %u rows without their column", n);
  if (int rc = usage_enter(c, "ydc_stream_usage_load")) return rc;
  if (!n && !add) return YDC_OK;
  auto& u = c->stream_mode.usage;
  // (every row may be a new key, and the next accrual's bound holds behind them)
  if (int rc = usage_fit(c, usage_bound(c->stream_mode) + n)) return rc;
  HIP_TRY(c, u.rows.reserve(std::max(n, 1u)));
  if (n) HIP_TRY(c, hipMemcpyAsync(u.rows.p, rows, (size_t)n * sizeof(UsageRow), hipMemcpyHostToDevice, c->stream));
  YDC_LAUNCH(c, "k_usage_load", k_usage_load, dim3(ceil_div(std::max(n, 1u), 256)), dim3(256), 0, c->stream, u.rows.p, n, u.tb,
             (unsigned long long)(add ? add->unattributed_time : 0), (unsigned long long)(add ? add->quanta : 0),
             (unsigned long long)(add ? add->ticks : 0));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  UsageState s{};
  HIP_TRY(c, hipMemcpy(&s, u.st.p, sizeof s, hipMemcpyDeviceToHost));
  if (s.dropped || s.n_keys > u.slots() / 2)
    return fail(c, YDC_ERR_NOT_CONVERGED, "usage: %u requestors in %u slots, %u additions dropped", s.n_keys, u.slots(), s.dropped);
  u.n_keys = s.n_keys;
  return YDC_OK;
}

int ydc_usage_quanta(int64_t last, int64_t now, int64_t quantum, uint64_t* out) {
  if (quantum <= 0 || !out) return YDC_ERR_INVALID_ARGUMENT;
  *out = usage_quanta(last, now, quantum);
  return YDC_OK;
}

// With withdrawal: the staged tags into the arena, sorted and without duplicates (the kernels search the
// list), each staged tag's place in that list kept for ydc_stream_withdraw_result; the staging consumed.
static void stream_withdraw_stage_tick(ydc_context::Stream& sm) {
  auto& w = sm.withdraw.host;
  std::vector<uint64_t> sorted(w.staged ? w.tags : std::vector<uint64_t>{});
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  w.place.resize(w.staged ? w.tags.size() : 0);
  for (size_t i = 0; i < w.place.size(); ++i)
    w.place[i] = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), w.tags[i]) - sorted.begin());
  w.n_unique = (uint32_t)sorted.size();
  w.counts.assign(w.n_unique, 0);
  if (w.n_unique) std::memcpy(sm.h.wd_tag, sorted.data(), (size_t)w.n_unique * 8);
  *sm.h.wd_n = w.n_unique;
  w.staged = false;
  w.tags.clear();
}

// With departure: the staged requestors into the arena, sorted and without duplicates (the kernels search
// the list), each staged requestor's place in that list kept for ydc_stream_depart_result; the staging
// consumed.
static void stream_depart_stage_tick(ydc_context::Stream& sm) {
  auto& d = sm.depart.host;
  if (!d.staged) d.ips.clear();
  std::vector<uint32_t> sorted(d.ips);
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  d.place.resize(d.ips.size());
  for (size_t i = 0; i < d.place.size(); ++i)
    d.place[i] = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), d.ips[i]) - sorted.begin());
  d.n_unique = (uint32_t)sorted.size();
  d.counts.assign(d.n_unique, make_uint4(0, 0, 0, 0));
  if (d.n_unique) std::memcpy(sm.h.dp_ip, sorted.data(), (size_t)d.n_unique * 4);
  *sm.h.dp_n = d.n_unique;
  d.asked = std::move(d.ips);
  d.ips.clear();
  d.staged = false;
}

// With a quota, in front of an accepted tick: the settings' device copy follows the host's (after a set,
// in a grown stream), and a table that a failed tick left behind is cleared. The stream is idle.
static int stream_quota_sync(ydc_context* c) {
  auto& q = c->stream_mode.quota;
  auto& h = q.host;
  if (h.table_dirty) {
    HIP_TRY(c, hipMemset(q.tb.word, 0, ((size_t)q.tb.mask + 1) * 8));
    // (... and so are ask[] and the sums of the fair-share level, which k_fair_level may not have cleared)
    HIP_TRY(c, hipMemset(q.fair.ask, 0, ((size_t)q.tb.mask + 1) * 4));
    HIP_TRY(c, hipMemset(q.fair.sums, 0, sizeof(FairSums)));
    h.table_dirty = false;
  }
  if (!h.dirty) return YDC_OK;
  const FairSet set{h.fair_mode, h.fair_pool, h.fair_floor, 0};
  HIP_TRY(c, hipMemcpy(const_cast<FairSet*>(q.fair.set), &set, sizeof set, hipMemcpyHostToDevice));
  const uint32_t n = (uint32_t)h.ip.size();
  if (n > q.max_overrides) return fail(c, YDC_ERR_NOT_CONVERGED, "%u overrides > max_overrides %u", n, q.max_overrides);
  if (n) {
    HIP_TRY(c, hipMemcpy(const_cast<uint32_t*>(q.caps.ip), h.ip.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(const_cast<uint32_t*>(q.caps.cap), h.cap.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  const uint32_t hdr[2] = {h.default_cap, n};
  HIP_TRY(c, hipMemcpy(const_cast<uint32_t*>(q.caps.hdr), hdr, sizeof hdr, hipMemcpyHostToDevice));
  h.dirty = false;
  return YDC_OK;
}

// Step 4: the tick into the arena (padding = no-ops), the staged columns consumed, the lease header
// and the tick number written.
static void stream_tick_stage(ydc_context* c, const StreamCall& t, const TickState& ts) {
  auto& sm = c->stream_mode;
  const TickArena& h = sm.h;
  const LeaseTick* lt = t.lt;
  const uint32_t graph_upd = ts.graph_upd, n_rel = t.n_rel, n_tasks = t.n_tasks, n_ids = ts.n_ids;
  // (a caller that filled the arena itself — ydc_stream_buffers_get — has nothing to copy)
  auto put = [](void* dst, const void* src, size_t n, size_t width) {
    if (n && src != dst) std::memcpy(dst, src, n * width);
  };
  put(h.upd_idx, t.upd_idx, graph_upd, 4);
  put(h.upd_rows, t.upd_rows, graph_upd, sizeof(ydc_servant_row));
  for (uint32_t i = graph_upd; i < sm.caps.max_updates; ++i) h.upd_idx[i] = 0xFFFFFFFFu;
  if (sm.alive.on) {  // (the staged expiries, consumed)
    put(h.upd_exp, sm.alive.stage.data(), graph_upd, 8);
    sm.alive.staged = false;
    sm.alive.stage.clear();
  }
  put(h.rel, t.rel, n_rel, 4);
  for (uint32_t i = n_rel; i < sm.caps.max_releases; ++i) h.rel[i] = 0xFFFFFFFFu;
  if (n_tasks) {
    put(h.env, t.tasks->env_id, n_tasks, 4);
    put(h.minv, t.tasks->min_version, n_tasks, 4);
    put(h.ip, t.tasks->requestor_ip, n_tasks, 4);
  }
  for (uint32_t i = n_tasks; i < sm.caps.max_tasks; ++i) {
    h.env[i] = 0xFFFFFFFFu;  // a digest nobody has: EnvironmentNotFound, consumes nothing
    h.minv[i] = 0;
    h.ip[i] = 0;
  }
  if (t.wt) {
    put(h.dl, t.wt->deadlines, n_tasks, 8);
    put(h.tag, t.wt->tags, n_tasks, 8);
    *h.now = t.wt->now;
  }
  if (lt) {
    put(h.lexp, lt->lease_exp, n_tasks, 8);
    put(h.ren_id, lt->renew_id, lt->n_renew, 8);
    put(h.ren_exp, lt->renew_exp, lt->n_renew, 8);
    put(h.free_id, lt->free_id, lt->n_free, 8);
    put(h.rep_srv, lt->rep_srv, lt->n_rep, 4);
    put(h.rep_off, lt->rep_off, lt->n_rep ? (size_t)lt->n_rep + 1 : 0, 4);
    put(h.rep_id, lt->rep_id, n_ids, 8);
    if (sm.max_book) {  // (the staged payload columns, consumed; nothing staged: zeros)
      if (sm.book.staged.on) {
        put(h.bk_stid, sm.book.staged.stid.data(), n_ids, 8);
        put(h.bk_dkey, sm.book.staged.dkey.data(), n_ids, 8);
      } else if (n_ids) {
        std::memset(h.bk_stid, 0, (size_t)n_ids * 8);
        std::memset(h.bk_dkey, 0, (size_t)n_ids * 8);
      }
      sm.book.staged.on = false;
      // (a report replaces its servant's entries, an empty one included: the digest index is stale)
      if (lt->n_rep) sm.book.index.valid = false;
    }
    // (the counts make the unused capacity a no-op; a tick number's low 30 bits are never 0)
    if ((++sm.lease_tick & kLeaseStamp) == 0) ++sm.lease_tick;
    *h.lh = LeaseHdr{lt->now, lt->n_renew, lt->n_free, lt->n_rep, n_ids, sm.lease_tick, 0};
  }
  if (sm.max_withdraw) stream_withdraw_stage_tick(sm);
  if (sm.max_depart) stream_depart_stage_tick(sm);
  if (sm.quota.on) *h.q_n = n_tasks;
  if (sm.usage.on && lt) {  // (the quanta since the previous accepted tick: the accrual's one word)
    auto& u = sm.usage;
    *u.h_dq = u.has_last ? usage_quanta(u.last, lt->now, u.quantum) : 0;
    u.last = lt->now;
    u.has_last = true;
  }
  if (t.rt) {
    put(h.nimm, t.rt->n_imm, n_tasks, 4);
    put(h.npre, t.rt->n_pre, n_tasks, 4);
    for (uint32_t i = n_tasks; i < sm.caps.max_tasks; ++i) h.nimm[i] = h.npre[i] = 0;  // (no rows: padding)
  }
}

// Step 5: the staged tick run — replayed from the captured step (stream_graph=0: enqueued), or
// enqueued eagerly where the step cannot be captured or its capture did not do.
static int stream_tick_run(ydc_context* c, const StreamCall& t, TickState* ts) {
  auto& sm = c->stream_mode;
  const bool wt = t.wt != nullptr, lt = t.lt != nullptr;
  // The ticks placed eagerly place this batch from the arena's device mirror. Waiting mode: the
  // batch is W's region + the new requests in HBM (k_wait_gather), its placement goes to wt_out
  // and k_wait_compact answers the caller.
  const ydc_task_soa batch_dev = wt ? ydc_task_soa{sm.wt.env, sm.wt.minv, sm.wt.ip}
                                    : ydc_task_soa{sm.d.env, sm.d.minv, sm.d.ip};
  uint32_t* const batch_out = wt ? sm.wt_out : lt ? sm.lt_out : c->d_out_idx.p;
  const uint32_t NB = stream_batch_n(sm);
  // (whatever of the tick is placed eagerly: COMMIT by copy, the stream being open)
  const BatchCall eager = batch_call(c, YDC_DISPATCH_COMMIT, batch_out, nullptr, nullptr, c->h_prm.dev());
  ts->plan = &ts->eager;
  if (sm.eager_only) {
    // The same step, enqueued instead of replayed: mirror the arena, apply, gather, place, answer.
    // (> kMaxWaveClasses classes: the bin sort, which needs at most that many, is never planned,
    // so place_batch never repeats the batch here)
    HIP_TRY(c, hipMemcpyAsync(sm.d_in.p, sm.h_in.p, sm.in_bytes, hipMemcpyHostToDevice, c->stream));
    if (lt) enqueue_lease_pre(c, sm.d);
    enqueue_apply_tick(c, sm.d);
    if (wt) enqueue_stream_gather(c, sm.d);
    if (int rc = place_batch(c, NB, &batch_dev, eager, &ts->eager, &ts->rounds))
      return rc;
    if (int rc = stream_answer_eager(c, sm.d)) return rc;
    // (profiling: the enqueued step names its launches, from the batch's front on — ydc_kernel_profile)
    if (c->profiling) collect_kernel_profile(c);
    return YDC_OK;
  }
  const bool second = sm.swaps && c->d_running.p == sm.run_b;
  if (sm.swaps && !second && c->d_running.p != sm.run_a)
    return fail(c, YDC_ERR_NOT_CONVERGED, "streaming: the running_tasks column is neither of the captured ones");
  if (c->opt_stream_graph) {
    HIP_TRY(c, hipGraphLaunch(second ? sm.exec_b : sm.exec, c->stream));
  } else {
    // (measurement, stream_graph=0: the same step enqueued kernel by kernel instead of replayed)
    const bool was_profiling = c->profiling;
    c->profiling = false;
    const int erc = stream_enqueue_step(c, second ? sm.plan_b : sm.plan, sm.swaps);
    c->profiling = was_profiling;
    if (erc) return erc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  const BatchPlan& p = second ? sm.plan_b : sm.plan;
  // (a step that took effect left the registry's running_tasks in its output column)
  if (sm.swaps && !c->h_prm->overflow && !(p.binsort && c->h_prm->window_miss) &&
      (!p.wave_path || c->h_prm->n_changed[(sm.passes - 1) & 63] == 0))
    std::swap(c->d_running, c->d_running_out);
  if (c->h_prm->overflow)
    return fail(c, YDC_ERR_CAPACITY, "slot workspace overflow (bound %u)", p.slot_bound);
  uint32_t rounds = sm.passes;
  if (p.binsort && c->h_prm->window_miss) {
    // A bin of the bin sort overflowed (bin_sort.h): the tick's registry deltas are applied, its
    // batch was gated out. Place it eagerly with the radix sort; the step is captured again,
    // without the bin sort, on the next tick.
    note_bin_overflow(c);
    // (the captured step read the arena in place: the device copy is stale; in waiting mode the
    // gathered batch in HBM is what is placed again, and W is still as the gather read it)
    HIP_TRY(c, hipMemcpyAsync(sm.d_in.p, sm.h_in.p, sm.in_bytes, hipMemcpyHostToDevice, c->stream));
    ts->rounds = rounds;
    if (int rc = place_batch(c, NB, &batch_dev, eager, &ts->eager, &ts->rounds))
      return rc;
    return stream_answer_eager(c, sm.d);
  }
  if (p.wave_path) {
    if (c->h_prm->n_changed[(sm.passes - 1) & 63] != 0) {
      // The captured passes were not enough (rare): finish eagerly and capture a longer
      // step next time.
      if (int rc = run_passes_until_consistent(c, p, sm.passes, eager, &rounds)) return rc;
      if (int rc = stream_answer_eager(c, sm.z)) return rc;
      c->round_hint = rounds;
      sm.want_passes = std::min(rounds + 1, 12u);
      sm.stale = true;
    } else {
      for (uint32_t r = 0; r < sm.passes; ++r)
        if (c->h_prm->n_changed[r & 63] == 0) {
          rounds = r + 1;
          break;
        }
      sm.window_max = std::max(sm.window_max, rounds);
      if (++sm.window_ticks >= 64) {
        if (sm.window_max < sm.passes && sm.passes > 2) {
          sm.want_passes = std::max(2u, sm.window_max);
          sm.stale = true;
        }
        sm.window_max = sm.window_ticks = 0;
      }
    }
  }
  ts->plan = &p;
  ts->rounds = rounds;
  return YDC_OK;
}

// Step 6, the end of every tick: the statistics of the placement without the padding,
// waiting mode's resolved list, the answers to the caller.
static int stream_tick_finish(ydc_context* c, const StreamCall& t, const TickState& ts) {
  auto& sm = c->stream_mode;
  const uint32_t n_tasks = t.n_tasks;
  fill_stats(c, *ts.plan, ts.rounds);
  if (sm.max_withdraw) {  // (the label pass has stored the counts of the list it saw)
    auto& w = sm.withdraw.host;
    if (sm.withdraw.h_done->n != w.n_unique)
      return fail(c, YDC_ERR_NOT_CONVERGED, "withdrawal: counts of %u tags, %u staged", sm.withdraw.h_done->n, w.n_unique);
    std::copy_n(sm.withdraw.h_count, w.n_unique, w.counts.begin());
  }
  if (sm.max_depart) {  // (k_depart_done has stored the counts of the list it saw)
    auto& d = sm.depart.host;
    const DepartDone& dd = *sm.depart.h_done;
    if (dd.n != d.n_unique || dd.tick_no != sm.lease_tick)
      return fail(c, YDC_ERR_NOT_CONVERGED, "departure: counts of %u requestors of tick %u (expected %u, %u)", dd.n,
                  dd.tick_no, d.n_unique, sm.lease_tick);
    std::copy_n(sm.depart.h_count, d.n_unique, d.counts.begin());
  }
  if (sm.usage.on) {  // (the accrual's last workgroup has stored the totals)
    auto& u = sm.usage;
    const UsageDone& d = *u.h_done;
    if (d.tick_no != sm.lease_tick)
      return fail(c, YDC_ERR_NOT_CONVERGED, "usage: result of tick %u (expected %u)", d.tick_no, sm.lease_tick);
    u.n_keys = d.n_keys;
    // What L and W gained in this tick came with its new requests. A tick that claimed nothing (dq == 0)
    // has left the keys of the ticks before it unclaimed: their allowance stays and this tick's joins it.
    u.fresh = (*u.h_dq ? 0 : u.fresh) + n_tasks;
    if (d.dropped || d.n_keys > u.slots() / 2)
      return fail(c, YDC_ERR_NOT_CONVERGED, "usage: %u keys in %u slots, %u additions dropped", d.n_keys, u.slots(), d.dropped);
  }
  uint32_t n_refused = 0;
  if (sm.quota.on) {  // (the label pass has stored what the clip admitted)
    auto& q = sm.quota;
    const QuotaDone& d = *q.h_done;
    if (d.tick_no != sm.lease_tick || d.n != n_tasks)
      return fail(c, YDC_ERR_NOT_CONVERGED, "quota: result of tick %u with %u requests (expected %u, %u)", d.tick_no, d.n,
                  sm.lease_tick, n_tasks);
    q.host.imm.assign(q.h_imm, q.h_imm + n_tasks);
    if (t.rt) q.host.pre.assign(q.h_pre, q.h_pre + n_tasks);
    q.host.rows_clipped = d.rows_clipped;
    q.host.n_refused = n_refused = d.n_refused;
    if (q.fair_on()) {  // (k_fair_done has stored the level's result block)
      const FairResult& f = *q.h_fres;
      if (f.tick_no != sm.lease_tick || f.mode != q.host.fair_mode)
        return fail(c, YDC_ERR_NOT_CONVERGED, "fair share: result of tick %u in mode %u (expected %u, %u)", f.tick_no, f.mode,
                    sm.lease_tick, q.host.fair_mode);
      q.host.fair_res = f;
    } else {
      q.host.fair_res = FairResult{};
      q.host.fair_res.tick_no = sm.lease_tick;
    }
  }
  if (t.rt) return stream_rpc_finish(c, t, ts);
  c->stats.n_tasks = n_tasks;
  c->stats.env_not_found -= std::min(c->stats.env_not_found, sm.caps.max_tasks - n_tasks);  // padding
  if (t.wt)
    if (int rc = stream_wait_finish(c, t.wt, n_tasks)) return rc;
  if (t.lt)
    if (int rc = stream_lease_finish(c, t.lt, n_tasks, ts.n_ids)) return rc;
  if (n_refused) {  // (a refused request was placed as padding: the statistics are those of a tick without it)
    c->stats.n_tasks -= std::min(c->stats.n_tasks, n_refused);
    c->stats.env_not_found -= std::min(c->stats.env_not_found, n_refused);
  }
  if (n_tasks && t.out_servant_idx != sm.h_out) std::memcpy(t.out_servant_idx, sm.h_out, (size_t)n_tasks * 4);
  return YDC_OK;
}

// (t by value: the removal route points it at the renumbered releases and reports)
static int stream_tick(ydc_context* c, StreamCall t) {
  if (!c || !c->stream_mode.active) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  TickState ts{c};
  if (int rc = stream_tick_check(c, t, &ts)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (sm.usage.on)  // (in front of everything the tick applies: a table that cannot grow refuses it)
    if (int rc = usage_fit(c, usage_bound(sm))) return rc;
  if (int rc = stream_tick_heartbeats(c, t, &ts)) return rc;
  if (sm.alive.on)
    if (int rc = stream_tick_expiry(c, t, &ts)) return rc;
  if (sm.stale || c->tables_dirty)
    if (int rc = stream_capture(c)) return rc;
  if (sm.quota.on)
    if (int rc = stream_quota_sync(c)) return rc;
  stream_tick_stage(c, t, ts);
  if (int rc = stream_tick_run(c, t, &ts)) {
    sm.quota.host.table_dirty = sm.quota.on;  // (its label pass may not have run)
    return rc;
  }
  if (ts.parked) {  // (behind a removal the parked leases go first)
    ts.parked = false;
    if (int rc = alive_orphans(c)) return rc;
  }
  return stream_tick_finish(c, t, ts);
}

int ydc_stream_tick_wide(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                         const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                         const uint32_t* release_servant_idx, uint32_t n_rel, const ydc_task_soa* tasks,
                         uint32_t n_tasks, uint32_t* out_servant_idx) {
  return stream_tick(c, StreamCall{upd_idx, upd_rows, upd_env_masks, env_words, n_upd, release_servant_idx, n_rel, tasks,
                                   n_tasks, out_servant_idx, nullptr, nullptr, nullptr});
}

int ydc_stream_begin_leased(ydc_context* c, uint32_t max_updates, uint32_t max_releases, uint32_t max_tasks,
                            uint32_t max_leases, uint32_t max_renewals, uint32_t max_frees, uint32_t max_reports,
                            uint32_t max_report_ids) {
  if (!c || !max_leases) return YDC_ERR_INVALID_ARGUMENT;
  return stream_begin(c, ydc_stream_caps{max_updates, max_releases, max_tasks, 0, 0, max_leases, max_renewals, max_frees,
                                         max_reports, max_report_ids});
}

int ydc_stream_tick_leased(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                           const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                           const uint32_t* release_servant_idx, uint32_t n_rel, const uint64_t* renew_task_id,
                           const int64_t* renew_expires_at, uint32_t n_renew, const uint64_t* free_task_id,
                           uint32_t n_free, const uint32_t* report_servant_idx, const uint32_t* report_off,
                           const uint64_t* report_task_id, uint32_t n_rep, const ydc_task_soa* tasks,
                           const int64_t* lease_expires_at, uint32_t n_tasks, int64_t now,
                           uint32_t* out_servant_idx, uint64_t* out_task_id, uint8_t* out_renewed,
                           uint8_t* out_report_unknown, uint32_t* out_n_leases) {
  const LeaseTick lt{renew_task_id, renew_expires_at, n_renew, free_task_id, n_free, report_servant_idx,
                     report_off, report_task_id, n_rep, lease_expires_at, now, out_task_id, out_renewed,
                     out_report_unknown, out_n_leases};
  return stream_tick(c, StreamCall{upd_idx, upd_rows, upd_env_masks, env_words, n_upd, release_servant_idx, n_rel, tasks,
                                   n_tasks, out_servant_idx, nullptr, &lt, nullptr});
}

int ydc_stream_begin_waiting_leased(ydc_context* c, uint32_t max_updates, uint32_t max_releases, uint32_t max_tasks,
                                    uint32_t max_waiting, uint32_t max_leases, uint32_t max_renewals,
                                    uint32_t max_frees, uint32_t max_reports, uint32_t max_report_ids) {
  if (!c || !max_waiting || !max_leases) return YDC_ERR_INVALID_ARGUMENT;
  return stream_begin(c, ydc_stream_caps{max_updates, max_releases, max_tasks, 0, max_waiting, max_leases, max_renewals,
                                         max_frees, max_reports, max_report_ids});
}

int ydc_stream_tick_waiting_leased(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                                   const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                                   const uint32_t* release_servant_idx, uint32_t n_rel,
                                   const uint64_t* renew_task_id, const int64_t* renew_expires_at, uint32_t n_renew,
                                   const uint64_t* free_task_id, uint32_t n_free,
                                   const uint32_t* report_servant_idx, const uint32_t* report_off,
                                   const uint64_t* report_task_id, uint32_t n_rep, const ydc_task_soa* tasks,
                                   const int64_t* lease_for, const int64_t* deadlines, const uint64_t* tags,
                                   uint32_t n_tasks, int64_t now, uint32_t* out_servant_idx, uint64_t* out_task_id,
                                   uint8_t* out_renewed, uint8_t* out_report_unknown, uint32_t* out_n_leases,
                                   uint64_t* out_resolved_tags, uint32_t* out_resolved_idx,
                                   uint64_t* out_resolved_task_id, uint32_t* out_n_resolved,
                                   uint32_t* out_n_waiting) {
  // (lease_for travels where a leased tick's absolute expiries do: the arena's per-request column)
  const LeaseTick lt{renew_task_id, renew_expires_at, n_renew, free_task_id, n_free, report_servant_idx,
                     report_off, report_task_id, n_rep, lease_for, now, out_task_id, out_renewed,
                     out_report_unknown, out_n_leases};
  const WaitTick wt{deadlines, tags, now, out_resolved_tags, out_resolved_idx, out_n_resolved, out_n_waiting,
                    out_resolved_task_id};
  return stream_tick(c, StreamCall{upd_idx, upd_rows, upd_env_masks, env_words, n_upd, release_servant_idx, n_rel, tasks,
                                   n_tasks, out_servant_idx, &wt, &lt, nullptr});
}

int ydc_stream_begin_rpc(ydc_context* c, uint32_t max_updates, uint32_t max_releases, uint32_t max_requests,
                         uint32_t max_rows, uint32_t max_waiting, uint32_t max_leases, uint32_t max_renewals,
                         uint32_t max_frees, uint32_t max_reports, uint32_t max_report_ids) {
  if (!c || !max_requests || !max_rows || !max_waiting || !max_leases) return YDC_ERR_INVALID_ARGUMENT;
  return stream_begin(c, ydc_stream_caps{max_updates, max_releases, max_requests, max_rows, max_waiting, max_leases,
                                         max_renewals, max_frees, max_reports, max_report_ids});
}

int ydc_stream_tick_rpc(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                        const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                        const uint32_t* release_servant_idx, uint32_t n_rel, const uint64_t* renew_task_id,
                        const int64_t* renew_expires_at, uint32_t n_renew, const uint64_t* free_task_id,
                        uint32_t n_free, const uint32_t* report_servant_idx, const uint32_t* report_off,
                        const uint64_t* report_task_id, uint32_t n_rep, const ydc_task_soa* requests,
                        const uint32_t* n_immediate, const uint32_t* n_prefetch, const int64_t* lease_for,
                        const int64_t* deadlines, const uint64_t* tags, uint32_t n_req, int64_t now,
                        uint32_t* out_status, uint32_t* out_n_granted, uint32_t* out_servant_idx,
                        uint64_t* out_task_id, uint8_t* out_renewed, uint8_t* out_report_unknown,
                        uint32_t* out_n_leases, uint64_t* out_resolved_tags, uint32_t* out_resolved_status,
                        uint32_t* out_resolved_n_granted, uint32_t* out_resolved_first,
                        uint32_t* out_resolved_servant_idx, uint64_t* out_resolved_task_id,
                        uint32_t* out_n_resolved, uint32_t* out_n_waiting, uint32_t* out_n_waiting_rows) {
  const LeaseTick lt{renew_task_id, renew_expires_at, n_renew, free_task_id, n_free, report_servant_idx,
                     report_off, report_task_id, n_rep, lease_for, now, out_task_id, out_renewed,
                     out_report_unknown, out_n_leases};
  const WaitTick wt{deadlines, tags, now, out_resolved_tags, out_resolved_status, out_n_resolved, out_n_waiting,
                    out_resolved_task_id};
  const RpcTick rt{n_immediate, n_prefetch, out_status, out_n_granted, out_resolved_n_granted, out_resolved_first,
                   out_resolved_servant_idx, out_n_waiting_rows};
  return stream_tick(c, StreamCall{upd_idx, upd_rows, upd_env_masks, env_words, n_upd, release_servant_idx, n_rel,
                                   requests, n_req, out_servant_idx, &wt, &lt, &rt});
}

// The table as it is, in id order: one copy of the columns, the live slots picked and sorted here.
int ydc_stream_leases_get(ydc_context* c, uint64_t* out_task_id, uint32_t* out_servant_idx,
                          int64_t* out_expires_at, uint8_t* out_zombie, uint32_t cap, uint32_t* out_n) {
  if (!c || !out_n || !c->stream_mode.active || !c->stream_mode.leased()) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t slots = (size_t)sm.lt.mask + 1;
  std::vector<unsigned long long> key(slots);
  std::vector<int64_t> exp(slots);
  std::vector<uint32_t> srv(slots), st(slots);
  HIP_TRY(c, hipMemcpy(key.data(), sm.lt.key, slots * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(exp.data(), sm.lt.expires, slots * 8, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(srv.data(), sm.lt.servant, slots * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(st.data(), sm.lt.state, slots * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> live;
  for (size_t i = 0; i < slots; ++i)
    if (st[i] & kLeaseLive) live.push_back((uint32_t)i);
  std::sort(live.begin(), live.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  *out_n = (uint32_t)live.size();
  if (live.size() > cap) return fail(c, YDC_ERR_CAPACITY, "%zu leases > cap %u", live.size(), cap);
  if (!live.empty() && (!out_task_id || !out_servant_idx || !out_expires_at || !out_zombie))
    return YDC_ERR_INVALID_ARGUMENT;
  for (size_t k = 0; k < live.size(); ++k) {
    const uint32_t i = live[k];
    out_task_id[k] = key[i];
    out_servant_idx[k] = srv[i];
    out_expires_at[k] = exp[i];
    out_zombie[k] = (st[i] & kLeaseZombie) ? 1 : 0;
  }
  return YDC_OK;
}

int ydc_stream_tick_waiting(ydc_context* c, const uint32_t* upd_idx, const ydc_servant_row* upd_rows,
                            const uint64_t* upd_env_masks, uint32_t env_words, uint32_t n_upd,
                            const uint32_t* release_servant_idx, uint32_t n_rel, const ydc_task_soa* tasks,
                            const int64_t* deadlines, const uint64_t* tags, uint32_t n_tasks, int64_t now,
                            uint32_t* out_servant_idx, uint64_t* out_resolved_tags, uint32_t* out_resolved_idx,
                            uint32_t* out_n_resolved, uint32_t* out_n_waiting) {
  const WaitTick wt{deadlines, tags, now, out_resolved_tags, out_resolved_idx, out_n_resolved, out_n_waiting,
                    nullptr};
  return stream_tick(c, StreamCall{upd_idx, upd_rows, upd_env_masks, env_words, n_upd, release_servant_idx, n_rel, tasks,
                                   n_tasks, out_servant_idx, &wt, nullptr, nullptr});
}

}  // extern "C"

// ---- snapshot and restore of an open stream (stream_snapshot.h, stream_snapshot_codec.h) ----
namespace {

// What the open stream holds, from the host's mirrors alone: mode, bounds, counts and with them the
// blob's layout. next_id and alive_bound are the device's to say (stream_snapshot fills them in).
void snap_describe(const ydc_context* c, snap::Header* h) {
  const auto& sm = c->stream_mode;
  std::memset(h, 0, sizeof *h);
  h->magic = snap::kMagic;
  h->version = snap::kVersion;
  h->mode = (sm.waiting() ? snap::kModeWaiting : 0) | (sm.leased() ? snap::kModeLeased : 0) |
            (sm.rpc() ? snap::kModeRpc : 0) | (sm.max_book ? snap::kModeBook : 0) | (sm.alive.on ? snap::kModeAlive : 0);
  h->env_words = c->reg.env_words;
  h->n_servants = c->reg.n;
  h->n_alias = (uint32_t)c->reg.alias_ip.size();
  for (int i = 0; i < snap::kCaps; ++i) h->caps[i] = sm.caps.*kCapFields[i];
  h->max_book = sm.max_book;
  h->n_leases = sm.leased() ? sm.n_leases : 0;
  h->n_waiting = sm.waiting() ? sm.n_waiting : 0;
  h->n_wait_rows = sm.rpc() ? sm.n_wait_rows : 0;
  h->n_book = sm.max_book ? sm.book.n : 0;
  h->lease_tick = sm.leased() ? sm.lease_tick : 0;
  h->last_now = sm.last_now;
  h->alive_bound = INT64_MAX;
  snap::layout(h);
}

// The four packed columns of L on the device, `cap` records each.
struct PackedBufs {
  DevBuf<unsigned long long> id;
  DevBuf<int64_t> exp;
  DevBuf<uint32_t> srv, st, count;
  LeasePacked cols{};
  hipError_t reserve(uint32_t cap) {
    for (hipError_t e : {id.reserve(cap), exp.reserve(cap), srv.reserve(cap), st.reserve(cap), count.reserve(1)})
      if (e != hipSuccess) return e;
    cols = LeasePacked{id.p, exp.p, srv.p, st.p, cap};
    return hipSuccess;
  }
};

int stream_snapshot(ydc_context* c, uint8_t* out, const snap::Header& h0) {
  auto& sm = c->stream_mode;
  snap::Header h = h0;
  snap::View v{};
  v.h = h;
  snap::place(&v, out);
  auto at = [](const uint8_t* col) { return const_cast<uint8_t*>(col); };  // (the view's columns lie in `out`)
  std::memset(out, 0, (size_t)h.total_bytes);
  hipStream_t st = c->stream;
  const uint32_t n = h.n_servants;
  // The registry: the device's columns are the truth for everything a heartbeat row replaces inside a
  // step (k_apply_tick leaves the winner of two rows for one servant undefined; mirror_rows takes the
  // last) and for running_tasks. ip_id and the environment masks change on the structural path only,
  // which writes the host's copy first; per servant, the device holds neither.
  if (n) {
    std::memcpy(at(v.env_mask), c->reg.env.data(), (size_t)n * h.env_words * 8);
    std::memcpy(at(v.ip), c->reg.ip.data(), (size_t)n * 4);
    for (auto& col : kRegCols)
      HIP_TRY(c, hipMemcpyAsync(at(v.*col.snap), (c->*col.dev).p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    // (rows behind the column's end have not reported yet: 0, which no tick number is)
    const uint32_t have = (uint32_t)std::min<size_t>(n, sm.d_rep_tick.cap);
    if (have) HIP_TRY(c, hipMemcpyAsync(at(v.rep_tick), sm.d_rep_tick.p, (size_t)have * 4, hipMemcpyDeviceToHost, st));
  }
  if (h.n_alias) {
    std::memcpy(at(v.alias_ip), c->reg.alias_ip.data(), (size_t)h.n_alias * 4);
    std::memcpy(at(v.alias_servant), c->reg.alias_servant.data(), (size_t)h.n_alias * 4);
  }
  // W, B, E: compact between ticks, [0, n) of every column as it lies.
  if (sm.waiting()) {
    uint32_t cnt = 0;
    HIP_TRY(c, hipMemcpy(&cnt, &sm.ws->count, 4, hipMemcpyDeviceToHost));
    if (cnt != h.n_waiting)
      return fail(c, YDC_ERR_NOT_CONVERGED, "waiting queue of %u on the device, %u on the host", cnt, h.n_waiting);
    const auto from = w_cols(sm);
    const auto to = w_cols(v);
    for (size_t k = 0; k < kWCols; ++k)
      if (cnt && from[k].p)
        HIP_TRY(c, hipMemcpyAsync(at(to[k]), from[k].p, cnt * from[k].width, hipMemcpyDeviceToHost, st));
  }
  if (h.n_book) {
    const auto from = b_cols(sm);
    const auto to = b_cols(v);
    for (size_t k = 0; k < kBCols; ++k)
      HIP_TRY(c, hipMemcpyAsync(at(to[k]), from[k].p, h.n_book * from[k].width, hipMemcpyDeviceToHost, st));
  }
  if (sm.alive.on && n) HIP_TRY(c, hipMemcpyAsync(at(v.e_exp), sm.alive.col.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  // L: packed on the device, brought over through one page-locked block (the four columns behind each
  // other), sorted by id here.
  if (sm.leased()) {
    const uint32_t nl = h.n_leases;
    const size_t cap = std::max(nl, 1u);
    HIP_TRY(c, c->d_snap.reserve(cap * 24 + 16));
    if (c->h_snap.cap < cap * 24)  // (a quarter more: |L| moves from snapshot to snapshot)
      HIP_TRY(c, c->h_snap.reserve(cap * 24 + cap * 6, hipHostMallocDefault));
    uint8_t* d = c->d_snap.p;
    const LeasePacked pk{(unsigned long long*)d, (int64_t*)(d + cap * 8), (uint32_t*)(d + cap * 16),
                         (uint32_t*)(d + cap * 20), (uint32_t)cap};
    uint32_t* d_count = (uint32_t*)(d + cap * 24);
    const uint8_t* stage = c->h_snap.p;
    HIP_TRY(c, hipMemsetAsync(d_count, 0, 4, st));
    YDC_LAUNCH(c, "k_lease_pack", k_lease_pack, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, st, sm.lt,
               pk, d_count);
    HIP_TRY(c, hipGetLastError());
    // (the copies of all |L| records are enqueued before the count is known to be |L|: the packed
    // columns hold that many, and a count that differs fails the call below)
    const unsigned long long* id = (const unsigned long long*)stage;
    const int64_t* exp = (const int64_t*)(stage + (size_t)nl * 8);
    const uint32_t* srv = (const uint32_t*)(stage + (size_t)nl * 16);
    const uint32_t* state = (const uint32_t*)(stage + (size_t)nl * 20);
    if (nl) {
      HIP_TRY(c, hipMemcpyAsync((void*)id, pk.id, (size_t)nl * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync((void*)exp, pk.expires, (size_t)nl * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync((void*)srv, pk.servant, (size_t)nl * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync((void*)state, pk.state, (size_t)nl * 4, hipMemcpyDeviceToHost, st));
    }
    LeaseState ls{};
    uint32_t packed = 0;
    HIP_TRY(c, hipMemcpyAsync(&packed, d_count, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&ls, sm.ls, sizeof ls, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (packed != nl || ls.n_leases != nl)
      return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u live slots, |L| %u on the device, %u on the host", packed,
                  ls.n_leases, nl);
    h.next_id = ls.next_id;
    std::vector<std::pair<unsigned long long, uint32_t>> order(nl);  // (id, packed position)
    for (uint32_t i = 0; i < nl; ++i) order[i] = {id[i], i};
    std::sort(order.begin(), order.end());
    for (uint32_t k = 0; k < nl; ++k) {
      const uint32_t i = order[k].second;
      // (between ticks no lease is parked: servant_alive.h)
      if (srv[i] >= n || id[i] >= ls.next_id)
        return fail(c, YDC_ERR_NOT_CONVERGED, "lease %llu names servant %u of %u (next_id %llu)", id[i], srv[i], n,
                    ls.next_id);
      std::memcpy(at(v.l_id) + (size_t)k * 8, &id[i], 8);
      std::memcpy(at(v.l_exp) + (size_t)k * 8, &exp[i], 8);
      std::memcpy(at(v.l_srv) + (size_t)k * 4, &srv[i], 4);
      std::memcpy(at(v.l_state) + (size_t)k * 4, &state[i], 4);
    }
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  // alive_bound: the column's minimum itself (the host's bound only errs low, by what it has seen).
  for (uint32_t s = 0; sm.alive.on && s < n; ++s) h.alive_bound = std::min(h.alive_bound, snap::get<int64_t>(v.e_exp, s));
  std::memcpy(out, &h, sizeof h);
  h.checksum = snap::checksum(out, h.total_bytes);
  std::memcpy(out, &h, sizeof h);
  return YDC_OK;
}

}  // namespace

extern "C" {

int ydc_stream_snapshot(ydc_context* c, void* out, size_t cap, size_t* out_bytes) {
  if (!c || !out_bytes) return YDC_ERR_INVALID_ARGUMENT;
  auto& sm = c->stream_mode;
  if (!sm.active) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_snapshot: no stream is open");
  if (!sm.waiting() && !sm.leased())
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_snapshot: a stream begun with ydc_stream_begin keeps no state "
                "on the device");
  if (c->group.n_ranks) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_snapshot: the context is in a group");
  if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_snapshot: pipelined batches are outstanding");
  if (sm.book.staged.on || sm.alive.staged || sm.withdraw.host.staged || sm.depart.host.staged)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_snapshot: a staging for the next tick is pending (a snapshot "
                "is taken between ticks)");
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (sm.alive.on)
    if (int rc = alive_fit(c)) return rc;  // (rows the registry gained outside a tick: "never")
  snap::Header h;
  snap_describe(c, &h);
  *out_bytes = (size_t)h.total_bytes;
  if (cap < h.total_bytes)
    return fail(c, YDC_ERR_CAPACITY, "a snapshot of %llu bytes > cap %zu", (unsigned long long)h.total_bytes, cap);
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  return stream_snapshot(c, (uint8_t*)out, h);
}

int ydc_stream_restore(ydc_context* c, const void* blob, size_t bytes, const ydc_stream_caps* want) {
  if (!c || !blob) return YDC_ERR_INVALID_ARGUMENT;
  if (c->group.n_ranks) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_restore: the context is in a group");
  if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_restore: pipelined batches are outstanding");
  // Everything that can be wrong with the bytes, before anything of the context is touched.
  snap::View v{};
  if (const char* why = snap::validate(blob, bytes, &v)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_restore: %s", why);
  const snap::Header& h = v.h;
  if (h.env_words > YDC_MAX_ENV_WORDS)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_restore: env_words %u > %u", h.env_words, YDC_MAX_ENV_WORDS);
  // (snap::validate has seen to it that the blob's bounds fit its mode bits: a part is there
  // exactly if its bound is not 0)
  ydc_stream_caps had{};
  for (int i = 0; i < snap::kCaps; ++i) had.*kCapFields[i] = h.caps[i];
  if (const char* why = want ? stream_caps_foreign(had, *want) : nullptr)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_restore: %s", why);
  const ydc_stream_caps k = want ? stream_caps_grown(had, *want) : had;
  if (int rc = stream_caps_check(c, YDC_ERR_INVALID_ARGUMENT, k, h.max_book)) return rc;
  if (c->max_servants && h.n_servants > c->max_servants)
    return fail(c, YDC_ERR_CAPACITY, "ydc_stream_restore: %u servants > max_servants %u", h.n_servants, c->max_servants);
  if (c->max_tasks && k.max_tasks > c->max_tasks)
    return fail(c, YDC_ERR_CAPACITY, "ydc_stream_restore: max_tasks %u > the context's %u", k.max_tasks, c->max_tasks);
  // The blob is good. From here on a failure is the device's (YDC_ERR_HIP, or a load that lost
  // records: YDC_ERR_NOT_CONVERGED) and leaves the blob's registry and no open stream.
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stream_release(c);
  const uint32_t n = h.n_servants;
  // (aligned copies of the columns: the block's base may be any address)
  auto col32 = [&](const uint8_t* p, size_t k) {
    std::vector<uint32_t> a(k);
    if (k) std::memcpy(a.data(), p, k * 4);
    return a;
  };
  auto col64 = [&](const uint8_t* p, size_t k) {
    std::vector<uint64_t> a(k);
    if (k) std::memcpy(a.data(), p, k * 8);
    return a;
  };
  {
    const auto version = col32(v.version, n), nproc = col32(v.nproc, n), load = col32(v.load, n);
    const auto maxt = col32(v.max_tasks, n), flags = col32(v.flags, n), ip = col32(v.ip, n), run = col32(v.running, n);
    const auto env = col64(v.env_mask, (size_t)n * h.env_words);
    const ydc_servant_soa sv{version.data(), nproc.data(), load.data(), maxt.data(), run.data(),
                             flags.data(), env.data(),  ip.data(),   h.env_words};
    if (int rc = ydc_upload_servants(c, &sv, n)) return rc;  // (registry and running_tasks; the aliases cleared)
    if (h.n_alias) {
      const auto aip = col32(v.alias_ip, h.n_alias), asv = col32(v.alias_servant, h.n_alias);
      if (int rc = ydc_set_host_aliases(c, aip.data(), asv.data(), h.n_alias)) return rc;
    }
  }
  // A second stream, complete before it becomes the context's.
  ydc_context::Stream fresh;
  auto load = [&]() -> int {
    if (int rc = stream_alloc(c, fresh, k, h.max_book, 0, 0, 0)) return rc;  // (withdrawal, the quota and departure stay off, like inspection)
    if (int rc = stream_reset(c, fresh)) return rc;
    hipStream_t st = c->stream;
    if (fresh.leased()) {
      const uint32_t nl = h.n_leases;
      PackedBufs pk;
      HIP_TRY(c, pk.reserve(std::max(nl, 1u)));
      if (nl) {
        HIP_TRY(c, hipMemcpy(pk.id.p, col64(v.l_id, nl).data(), (size_t)nl * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(pk.exp.p, col64(v.l_exp, nl).data(), (size_t)nl * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(pk.srv.p, col32(v.l_srv, nl).data(), (size_t)nl * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(pk.st.p, col32(v.l_state, nl).data(), (size_t)nl * 4, hipMemcpyHostToDevice));
      }
      YDC_LAUNCH(c, "k_lease_load", k_lease_load, dim3(ceil_div(std::max(nl, 1u), 256)), dim3(256), 0, st, fresh.lt,
                 fresh.ls, pk.cols, nl, (unsigned long long)h.next_id);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(st));
      LeaseState ls{};
      HIP_TRY(c, hipMemcpy(&ls, fresh.ls, sizeof ls, hipMemcpyDeviceToHost));
      if (ls.n_leases != nl || ls.next_id != h.next_id)
        return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u of %u leases filed (next_id %llu of %llu)", ls.n_leases,
                    nl, ls.next_id, (unsigned long long)h.next_id);
      // (sized by the registry, as stream_capture sizes it; rows that never reported: 0)
      HIP_TRY(c, fresh.d_rep_tick.reserve((size_t)n + 1024));
      HIP_TRY(c, hipMemset(fresh.d_rep_tick.p, 0, fresh.d_rep_tick.cap * 4));
      if (n) HIP_TRY(c, hipMemcpy(fresh.d_rep_tick.p, col32(v.rep_tick, n).data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (h.n_waiting) {
      // (pageable and unaligned sources: synchronous copies)
      const auto from = w_cols(v);
      const auto to = w_cols(fresh);
      for (size_t k = 0; k < kWCols; ++k)
        if (to[k].p) HIP_TRY(c, hipMemcpy(to[k].p, from[k], h.n_waiting * to[k].width, hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(&fresh.ws->count, &h.n_waiting, 4, hipMemcpyHostToDevice));
    }
    if (h.n_book) {
      const auto from = b_cols(v);
      const auto to = b_cols(fresh);
      for (size_t k = 0; k < kBCols; ++k)
        HIP_TRY(c, hipMemcpy(to[k].p, from[k], h.n_book * to[k].width, hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(&fresh.book.bks->n_entries, &h.n_book, 4, hipMemcpyHostToDevice));
    }
    if (h.mode & snap::kModeAlive) {  // (ydc_stream_alive_begin's allocation)
      HIP_TRY(c, fresh.alive.col.reserve((size_t)n + n / 2 + 1024));
      if (n) HIP_TRY(c, hipMemcpy(fresh.alive.col.p, v.e_exp, (size_t)n * 8, hipMemcpyHostToDevice));
      fresh.alive.on = true;
      fresh.alive.n = n;
      fresh.alive.bound = h.alive_bound;
    }
    // The host's mirrors. What a stream learns (want_passes and its window) and the per-tick marks
    // (rep_seen / rep_mark, alive_seen / alive_mark) start fresh: none of them outlives a tick in
    // anything a tick returns.
    fresh.n_waiting = h.n_waiting;
    fresh.n_wait_rows = h.n_wait_rows;
    fresh.n_leases = h.n_leases;
    fresh.book.n = h.n_book;
    fresh.last_now = h.last_now;
    fresh.lease_tick = h.lease_tick;
    return YDC_OK;
  };
  if (int rc = load()) {
    stream_release(fresh);
    return rc;
  }
  std::swap(c->stream_mode, fresh);  // (stale: the next tick captures its step)
  return YDC_OK;
}

}  // extern "C"

// ---- delta snapshots (stream_delta.h, stream_delta_codec.h) ----
namespace {

// A packed image of `cap` records in one buffer, the four columns behind each other.
LeasePacked packed_at(uint8_t* d, size_t cap) {
  return LeasePacked{(unsigned long long*)d, (int64_t*)(d + cap * 8), (uint32_t*)(d + cap * 16), (uint32_t*)(d + cap * 20),
                     (uint32_t)cap};
}

// The lists' scratch of the base: inserted | erased | updated | the counters.
struct DeltaLists {
  LeasePacked ins;
  unsigned long long* era;
  LeaseUpdates upd;
  DeltaCounts* cnt;
};
DeltaLists delta_lists(uint8_t* d, size_t cap) {
  uint8_t* u = d + cap * 32;
  return DeltaLists{packed_at(d, cap), (unsigned long long*)(d + cap * 24),
                    LeaseUpdates{(unsigned long long*)u, (int64_t*)(u + cap * 8), (uint32_t*)(u + cap * 16), (uint32_t)cap},
                    (DeltaCounts*)(d + cap * 52)};
}

// B's columns in the base's copy (max_book entries each, b_cols' order).
BookCols delta_book_at(uint8_t* d, size_t max_book) {
  return BookCols{(uint32_t*)(d + max_book * 24), (unsigned long long*)d, (unsigned long long*)(d + max_book * 8),
                  (unsigned long long*)(d + max_book * 16)};
}

// The structure stamp of the context as it is now (h: snap_describe's).
uint64_t delta_stamp(const ydc_context* c, const snap::Header& h) {
  return delta::stamp(h.mode, h.env_words, h.n_servants, h.n_alias, h.caps, h.max_book, c->reg.env.data(), c->reg.ip.data(),
                      c->reg.alias_ip.data(), c->reg.alias_servant.data());
}

// What all four calls refuse.
int delta_mode_check(ydc_context* c, const char* what) {
  const auto& sm = c->stream_mode;
  if (!sm.active) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: no stream is open", what);
  if (!sm.leased()) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the stream keeps no lease table", what);
  if (c->group.n_ranks) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the context is in a group", what);
  return YDC_OK;
}

// ... and what a snapshot refuses besides; then the stream is brought to rest as a snapshot does.
int delta_settle(ydc_context* c, const char* what) {
  auto& sm = c->stream_mode;
  if (c->pend_count) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: pipelined batches are outstanding", what);
  if (sm.book.staged.on || sm.alive.staged || sm.withdraw.host.staged || sm.depart.host.staged)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: a staging for the next tick is pending", what);
  HIP_TRY(c, hipSetDevice(c->device));
  resident_stop(c);  // (the registry leaves the resident kernel's registers)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (sm.alive.on)
    if (int rc = alive_fit(c)) return rc;
  return YDC_OK;
}

// B as it is now into the base's copy.
int delta_keep_book(ydc_context* c) {
  auto& sm = c->stream_mode;
  auto& b = sm.delta;
  b.n_book = sm.max_book ? sm.book.n : 0;
  if (!b.n_book) return YDC_OK;
  HIP_TRY(c, b.book.reserve((size_t)sm.max_book * 28));
  const BookCols to = delta_book_at(b.book.p, sm.max_book);
  const StateCol dst[kBCols] = {{to.grant, 8}, {to.stid, 8}, {to.dkey, 8}, {to.servant, 4}};
  const auto from = b_cols(sm);
  for (size_t k = 0; k < kBCols; ++k)
    HIP_TRY(c, hipMemcpyAsync(dst[k].p, from[k].p, b.n_book * from[k].width, hipMemcpyDeviceToDevice, c->stream));
  return YDC_OK;
}

// The base taken from the snapshot just written (h: its header): L's packed columns as k_lease_pack left
// them in d_snap, device to device.
int delta_take_base(ydc_context* c, const snap::Header& h) {
  auto& sm = c->stream_mode;
  auto& b = sm.delta;
  b.on = false;
  const size_t cap = sm.caps.max_leases;
  for (auto& im : b.img) HIP_TRY(c, im.reserve(cap * 24));
  HIP_TRY(c, b.lists.reserve(cap * 52 + sizeof(DeltaCounts)));
  b.cap = (uint32_t)cap;
  b.cur = 0;
  const uint32_t nl = h.n_leases;
  if (nl) {
    const LeasePacked from = packed_at(c->d_snap.p, std::max(nl, 1u)), to = packed_at(b.img[0].p, cap);
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemcpyAsync(to.id, from.id, (size_t)nl * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(to.expires, from.expires, (size_t)nl * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(to.servant, from.servant, (size_t)nl * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(to.state, from.state, (size_t)nl * 4, hipMemcpyDeviceToDevice, st));
  }
  if (int rc = delta_keep_book(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  b.n = nl;
  b.next_id = h.next_id;
  b.last_now = h.last_now;
  b.lease_tick = h.lease_tick;
  b.n_waiting = h.n_waiting;
  b.stamp = delta_stamp(c, h);
  b.on = true;
  return YDC_OK;
}

// One column of a list: where it lies on the device, where it goes in the blob, its width.
struct ListCol {
  const void* dev;
  uint8_t* to;
  size_t width;
};

int stream_delta(ydc_context* c, void* out, size_t cap, size_t* out_bytes) {
  auto& sm = c->stream_mode;
  auto& b = sm.delta;
  snap::Header sh;
  snap_describe(c, &sh);
  if (delta_stamp(c, sh) != b.stamp || sm.caps.max_leases != b.cap) {
    b = ydc_context::Stream::DeltaBase{};
    return fail(c, YDC_ERR_NO_BASE, "ydc_stream_delta: the registry's structure, the aliases, a bound or the mode changed "
                "since the base");
  }
  hipStream_t st = c->stream;
  const uint32_t n = sh.n_servants;
  const LeasePacked old_img = packed_at(b.img[b.cur].p, b.cap), new_img = packed_at(b.img[b.cur ^ 1].p, b.cap);
  const DeltaLists ls = delta_lists(b.lists.p, b.cap);
  HIP_TRY(c, hipMemsetAsync(ls.cnt, 0, sizeof(DeltaCounts), st));
  YDC_LAUNCH(c, "k_lease_delta_scan", k_lease_delta_scan, dim3(ceil_div(sm.lt.mask + 1, kLeaseTile)), dim3(256), 0, st,
             sm.lt, new_img, ls.ins, b.next_id, ls.cnt);
  HIP_TRY(c, hipGetLastError());
  YDC_LAUNCH(c, "k_lease_delta_diff", k_lease_delta_diff, dim3(ceil_div(std::max(b.n, 1u), 256)), dim3(256), 0, st, sm.lt,
             sm.ls, old_img, b.n, ls.era, b.cap, ls.upd, ls.cnt);
  HIP_TRY(c, hipGetLastError());
  const bool book_compared = sm.max_book && sm.book.n == b.n_book && b.n_book;
  if (book_compared) {
    YDC_LAUNCH(c, "k_book_delta_same", k_book_delta_same, dim3(ceil_div(b.n_book, 256)), dim3(256), 0, st, sm.book.bk,
               delta_book_at(b.book.p, sm.max_book), b.n_book, ls.cnt);
    HIP_TRY(c, hipGetLastError());
  }
  DeltaCounts cnt{};
  LeaseState lst{};
  uint32_t n_w = 0;
  HIP_TRY(c, hipMemcpyAsync(&cnt, ls.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&lst, sm.ls, sizeof lst, hipMemcpyDeviceToHost, st));
  if (sm.waiting()) HIP_TRY(c, hipMemcpyAsync(&n_w, &sm.ws->count, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (cnt.n_img != sh.n_leases || lst.n_leases != sh.n_leases)
    return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: %u live slots, |L| %u on the device, %u on the host", cnt.n_img,
                lst.n_leases, sh.n_leases);
  if (n_w != sh.n_waiting)
    return fail(c, YDC_ERR_NOT_CONVERGED, "waiting queue of %u on the device, %u on the host", n_w, sh.n_waiting);
  if (cnt.servant_changed)
    return fail(c, YDC_ERR_NOT_CONVERGED, "ydc_stream_delta: %u leases changed their servant under an equal structure stamp",
                cnt.servant_changed);
  if (cnt.n_era > b.n || cnt.n_upd > b.n - cnt.n_era || cnt.n_ins > cnt.n_img ||
      (uint64_t)b.n + cnt.n_ins - cnt.n_era != cnt.n_img || lst.next_id < b.next_id)
    return fail(c, YDC_ERR_NOT_CONVERGED, "ydc_stream_delta: %u inserted, %u erased, %u updated of %u do not make %u", cnt.n_ins,
                cnt.n_era, cnt.n_upd, b.n, cnt.n_img);
  // The header, and with it the size.
  snap::Header base_h{};
  base_h.next_id = b.next_id, base_h.last_now = b.last_now, base_h.lease_tick = b.lease_tick;
  base_h.n_leases = b.n, base_h.n_waiting = b.n_waiting;
  sh.next_id = lst.next_id;
  delta::Header h = delta::describe(base_h, sh, b.stamp);
  h.n_ins = cnt.n_ins, h.n_era = cnt.n_era, h.n_upd = cnt.n_upd;
  h.book_present = sm.max_book && (!book_compared ? sm.book.n != b.n_book : cnt.book_differs != 0);
  delta::layout(&h);
  *out_bytes = (size_t)h.total_bytes;
  if (cap < h.total_bytes)  // (the new image is simply not taken: the next call scans again)
    return fail(c, YDC_ERR_CAPACITY, "a delta of %llu bytes > cap %zu", (unsigned long long)h.total_bytes, cap);
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  uint8_t* o = (uint8_t*)out;
  std::memset(o, 0, (size_t)h.total_bytes);
  delta::View v{};
  v.h = h;
  delta::place(&v, o);
  auto at = [](const uint8_t* col) { return const_cast<uint8_t*>(col); };
  // The three lists: brought over as they lie, sorted by id here (they are small).
  auto sorted = [&](uint32_t k, const unsigned long long* d_id, std::initializer_list<ListCol> cols) -> int {
    if (!k) return YDC_OK;
    std::vector<unsigned long long> id(k);
    HIP_TRY(c, hipMemcpy(id.data(), d_id, (size_t)k * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> order(k);
    for (uint32_t i = 0; i < k; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return id[x] < id[y]; });
    std::vector<uint8_t> col;
    for (const ListCol& lc : cols) {
      col.resize((size_t)k * lc.width);
      HIP_TRY(c, hipMemcpy(col.data(), lc.dev, col.size(), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < k; ++i) std::memcpy(lc.to + (size_t)i * lc.width, &col[(size_t)order[i] * lc.width], lc.width);
    }
    return YDC_OK;
  };
  if (int rc = sorted(h.n_ins, ls.ins.id, {{ls.ins.id, at(v.ins_id), 8}, {ls.ins.expires, at(v.ins_exp), 8},
                                           {ls.ins.servant, at(v.ins_srv), 4}, {ls.ins.state, at(v.ins_state), 4}}))
    return rc;
  if (int rc = sorted(h.n_era, ls.era, {{ls.era, at(v.era_id), 8}})) return rc;
  if (int rc = sorted(h.n_upd, ls.upd.id, {{ls.upd.id, at(v.upd_id), 8}, {ls.upd.expires, at(v.upd_exp), 8},
                                           {ls.upd.state, at(v.upd_state), 4}}))
    return rc;
  for (uint32_t i = 0; i < h.n_ins; ++i)
    if (snap::get<uint32_t>(v.ins_srv, i) >= n)
      return fail(c, YDC_ERR_NOT_CONVERGED, "an inserted lease names servant %u of %u", snap::get<uint32_t>(v.ins_srv, i), n);
  // The registry's light columns (the device's are the truth: stream_snapshot), W, E and B, whole.
  if (n) {
    const uint32_t* reg[delta::kRegCols] = {c->d_version.p, c->d_nproc.p, c->d_load.p, c->d_max_tasks.p,
                                           c->d_flags.p,   c->d_running.p, nullptr};
    for (int k = 0; k + 1 < delta::kRegCols; ++k)
      HIP_TRY(c, hipMemcpyAsync(at(v.reg[k]), reg[k], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    const uint32_t have = (uint32_t)std::min<size_t>(n, sm.d_rep_tick.cap);
    if (have) HIP_TRY(c, hipMemcpyAsync(at(v.reg[6]), sm.d_rep_tick.p, (size_t)have * 4, hipMemcpyDeviceToHost, st));
  }
  if (sm.waiting() && n_w) {
    const auto from = w_cols(sm);
    const uint8_t* to[kWCols] = {v.w_deadline, v.w_tag, v.w_for, v.w_env, v.w_minv, v.w_ip, v.w_nimm, v.w_npre};
    for (size_t k = 0; k < kWCols; ++k)
      if (from[k].p) HIP_TRY(c, hipMemcpyAsync(at(to[k]), from[k].p, n_w * from[k].width, hipMemcpyDeviceToHost, st));
  }
  if (sm.alive.on && n) HIP_TRY(c, hipMemcpyAsync(at(v.e_exp), sm.alive.col.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (h.book_present && h.n_book) {
    const auto from = b_cols(sm);
    const uint8_t* to[kBCols] = {v.b_grant, v.b_stid, v.b_dkey, v.b_srv};
    for (size_t k = 0; k < kBCols; ++k)
      HIP_TRY(c, hipMemcpyAsync(at(to[k]), from[k].p, h.n_book * from[k].width, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  for (uint32_t s = 0; sm.alive.on && s < n; ++s) h.alive_bound = std::min(h.alive_bound, snap::get<int64_t>(v.e_exp, s));
  delta::seal(o, &h);
  // The current state is the new base.
  if (h.book_present)
    if (int rc = delta_keep_book(c)) {
      b = ydc_context::Stream::DeltaBase{};
      return rc;
    }
  HIP_TRY(c, hipStreamSynchronize(st));
  b.cur ^= 1;
  b.n = cnt.n_img;
  b.next_id = lst.next_id;
  b.last_now = sh.last_now;
  b.lease_tick = sh.lease_tick;
  b.n_waiting = sh.n_waiting;
  return YDC_OK;
}

// The body of ydc_stream_delta_apply and ydc_stream_delta_apply_inspected. `side`: the delta's inspection
// sidecar (validated, and checked against the delta by the caller), or nullptr on a stream without inspection.
int stream_delta_apply(ydc_context* c, const char* what, const delta::View& v, const insd::View* side) {
  auto& sm = c->stream_mode;
  const delta::Header& h = v.h;
  snap::Header sh;
  snap_describe(c, &sh);
  const uint32_t n = sh.n_servants;
  // The delta's base is this context's state.
  if (h.mode != sh.mode || h.env_words != sh.env_words || h.n_servants != n || h.max_leases != sm.caps.max_leases ||
      h.max_waiting != sm.caps.max_waiting || h.max_rows != sm.caps.max_rows || h.max_book != sm.max_book ||
      h.stamp != delta_stamp(c, sh))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the delta's structure stamp is not this context's", what);
  LeaseState lst{};
  HIP_TRY(c, hipMemcpy(&lst, sm.ls, sizeof lst, hipMemcpyDeviceToHost));
  if (h.base_lease_tick != sm.lease_tick || h.base_next_id != lst.next_id || h.base_n_leases != sm.n_leases ||
      lst.n_leases != sm.n_leases || h.base_n_waiting != sh.n_waiting || h.base_last_now != sm.last_now)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the delta's base (tick %u, next_id %llu, |L| %u, |W| %u) "
                "is not this context's state (tick %u, next_id %llu, |L| %u, |W| %u)", what, h.base_lease_tick,
                (unsigned long long)h.base_next_id, h.base_n_leases, h.base_n_waiting, sm.lease_tick, lst.next_id,
                sm.n_leases, sh.n_waiting);
  if (!h.book_present && sm.max_book && h.n_book != sm.book.n)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: |B| %u without B, %u here", what, h.n_book, sm.book.n);
  hipStream_t st = c->stream;
  // The lists on the device (aligned copies: the block's base may be any address), and the read-only
  // pass: every erased and updated id is in the table, no inserted one is.
  const size_t ni = h.n_ins, ne = h.n_era, nu = h.n_upd;
  const size_t o_ins = 0, o_era = ni * 24, o_upd = o_era + ne * 8, o_cnt = (o_upd + nu * 20 + 7) & ~(size_t)7;
  // (with a sidecar, its records behind the counters: started_at | env_id | requestor_ip | prefetch)
  const size_t o_rec = o_cnt + ((sizeof(DeltaCounts) + 7) & ~(size_t)7), rec_bytes = side ? ni * 17 : 0;
  std::vector<uint64_t> stage((o_rec + rec_bytes + 7) / 8, 0);  // (8-byte units; the counters behind the lists)
  uint8_t* s8 = (uint8_t*)stage.data();
  if (side && (sm.inspect.n != n || sm.inspect.disc.cap < n || sm.inspect.ever.cap < n))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the inspection columns have %u rows for %u servants", what, sm.inspect.n, n);
  std::memcpy(s8 + o_ins, v.ins_id, ni * 8);
  std::memcpy(s8 + o_ins + ni * 8, v.ins_exp, ni * 8);
  std::memcpy(s8 + o_ins + ni * 16, v.ins_srv, ni * 4);
  std::memcpy(s8 + o_ins + ni * 20, v.ins_state, ni * 4);
  std::memcpy(s8 + o_era, v.era_id, ne * 8);
  std::memcpy(s8 + o_upd, v.upd_id, nu * 8);
  std::memcpy(s8 + o_upd + nu * 8, v.upd_exp, nu * 8);
  std::memcpy(s8 + o_upd + nu * 16, v.upd_state, nu * 4);
  auto& buf = sm.delta.apply;
  HIP_TRY(c, buf.reserve(o_rec + rec_bytes));
  const InspectRecords recs{(int64_t*)(buf.p + o_rec), (uint32_t*)(buf.p + o_rec + ni * 8), (uint32_t*)(buf.p + o_rec + ni * 12),
                            buf.p + o_rec + ni * 16};
  if (side) {  // (lists, cleared counters and records in one copy)
    if (ni) std::memcpy(s8 + o_rec, side->started_at, ni * 17);  // (the record section's four columns lie like this)
    HIP_TRY(c, hipMemcpy(buf.p, s8, o_rec + rec_bytes, hipMemcpyHostToDevice));
  } else {
    if (o_cnt) HIP_TRY(c, hipMemcpy(buf.p, s8, o_cnt, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(buf.p + o_cnt, 0, sizeof(DeltaCounts)));
  }
  const LeasePacked ins = packed_at(buf.p + o_ins, ni);
  const unsigned long long* era = (const unsigned long long*)(buf.p + o_era);
  uint8_t* u = buf.p + o_upd;
  const LeaseUpdates upd{(unsigned long long*)u, (int64_t*)(u + nu * 8), (uint32_t*)(u + nu * 16), (uint32_t)nu};
  DeltaCounts* d_cnt = (DeltaCounts*)(buf.p + o_cnt);
  YDC_LAUNCH(c, "k_lease_delta_check", k_lease_delta_check, dim3(ceil_div((uint32_t)std::max<size_t>(ne + nu + ni, 1), 256)),
             dim3(256), 0, st, sm.lt, sm.ls, era, (uint32_t)ne, upd.id, (uint32_t)nu, ins.id, (uint32_t)ni, d_cnt);
  HIP_TRY(c, hipGetLastError());
  DeltaCounts cnt{};
  HIP_TRY(c, hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (cnt.found_old != ne + nu || cnt.found_new)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: %u of %zu erased and updated ids are leases here, and %u "
                "of the inserted ones", what, cnt.found_old, ne + nu, cnt.found_new);
  if (sm.d_rep_tick.cap < n) {  // (never after a restore, which sizes it by the registry; the step holds its address)
    DevBuf<uint32_t> bigger;
    HIP_TRY(c, bigger.reserve((size_t)n + 1024));
    sm.d_rep_tick = std::move(bigger);
    sm.stale = true;
  }
  // From here on the context is written. Usage goes off (a standby does not accrue: stream_usage.h); L first.
  if (sm.usage.on) {
    sm.usage = ydc_context::Stream::Usage{};
    sm.stale = true;
  }
  if (ne + nu) {
    YDC_LAUNCH(c, "k_lease_delta_apply_old", k_lease_delta_apply_old, dim3(ceil_div((uint32_t)(ne + nu), 256)), dim3(256), 0,
               st, sm.lt, sm.ls, era, (uint32_t)ne, upd, (uint32_t)nu);
    HIP_TRY(c, hipGetLastError());
  }
  if (side) {
    YDC_LAUNCH(c, "k_lease_delta_apply_inspect", k_lease_delta_apply_inspect,
               dim3(ceil_div((uint32_t)std::max<size_t>(ni, 1), 256)), dim3(256), 0, st, sm.lt, sm.ls, ins, recs, (uint32_t)ni,
               (unsigned long long)h.next_id, h.n_leases, sm.d_insp_rec.p, sm.d_insp_pre.p);
  } else {
    YDC_LAUNCH(c, "k_lease_delta_apply_new", k_lease_delta_apply_new, dim3(ceil_div((uint32_t)std::max<size_t>(ni, 1), 256)),
               dim3(256), 0, st, sm.lt, sm.ls, ins, (uint32_t)ni, (unsigned long long)h.next_id, h.n_leases);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  if (side && n) {  // (the two servant columns, whole, into buffers that stay where they are)
    HIP_TRY(c, hipMemcpy(sm.inspect.disc.p, side->discovered_at, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(sm.inspect.ever.p, side->ever_assigned, (size_t)n * 8, hipMemcpyHostToDevice));
  }
  // The registry's light columns, on the device and in the host's mirror. Rows whose version or
  // capacity bound moved (a structural turn the stamp does not cover) have the derived tables rebuilt.
  bool structural = false;
  if (n) {
    uint32_t* dev[delta::kRegCols] = {c->d_version.p, c->d_nproc.p, c->d_load.p, c->d_max_tasks.p,
                                     c->d_flags.p,   c->d_running.p, sm.d_rep_tick.p};
    for (int k = 0; k < delta::kRegCols; ++k) HIP_TRY(c, hipMemcpy(dev[k], v.reg[k], (size_t)n * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> version(n), nproc(n), maxt(n);
    std::memcpy(version.data(), v.reg[0], (size_t)n * 4);
    std::memcpy(nproc.data(), v.reg[1], (size_t)n * 4);
    std::memcpy(maxt.data(), v.reg[3], (size_t)n * 4);
    auto& r = c->reg;
    for (uint32_t s = 0; s < n && !structural; ++s)
      structural = version[s] != r.version[s] || (maxt[s] == 0) != (r.max_tasks[s] == 0) ||
                   std::min(maxt[s], nproc[s]) != std::min(r.max_tasks[s], r.nproc[s]);
    r.version = std::move(version), r.nproc = std::move(nproc), r.max_tasks = std::move(maxt);
    std::memcpy(r.load.data(), v.reg[2], (size_t)n * 4);
    std::memcpy(r.flags.data(), v.reg[4], (size_t)n * 4);
  }
  // W, E and B: plain copies (pageable and unaligned sources: synchronous ones).
  if (sm.waiting()) {
    const uint8_t* from[kWCols] = {v.w_deadline, v.w_tag, v.w_for, v.w_env, v.w_minv, v.w_ip, v.w_nimm, v.w_npre};
    const auto to = w_cols(sm);
    for (size_t k = 0; h.n_waiting && k < kWCols; ++k)
      if (to[k].p) HIP_TRY(c, hipMemcpy(to[k].p, from[k], h.n_waiting * to[k].width, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(&sm.ws->count, &h.n_waiting, 4, hipMemcpyHostToDevice));
    sm.n_waiting = h.n_waiting;
    sm.n_wait_rows = h.n_wait_rows;
  }
  if (sm.alive.on) {
    if (n) HIP_TRY(c, hipMemcpy(sm.alive.col.p, v.e_exp, (size_t)n * 8, hipMemcpyHostToDevice));
    sm.alive.n = n;
    sm.alive.bound = h.alive_bound;
  }
  if (h.book_present) {
    const uint8_t* from[kBCols] = {v.b_grant, v.b_stid, v.b_dkey, v.b_srv};
    const auto to = b_cols(sm);
    for (size_t k = 0; h.n_book && k < kBCols; ++k)
      HIP_TRY(c, hipMemcpy(to[k].p, from[k], h.n_book * to[k].width, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(&sm.book.bks->n_entries, &h.n_book, 4, hipMemcpyHostToDevice));
    sm.book.n = h.n_book;
    sm.book.index.valid = false;
  }
  sm.n_leases = h.n_leases;
  sm.last_now = h.last_now;
  sm.lease_tick = h.lease_tick;
  if (structural) return rebuild_tables(c);
  return YDC_OK;
}

}  // namespace

extern "C" {

int ydc_stream_delta_base(ydc_context* c, void* out, size_t cap, size_t* out_bytes) {
  if (!c || !out_bytes) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = delta_mode_check(c, "ydc_stream_delta_base")) return rc;
  if (int rc = ydc_stream_snapshot(c, out, cap, out_bytes)) return rc;  // (refused: the base, if any, stays)
  snap::Header h;
  std::memcpy(&h, out, sizeof h);
  if (int rc = delta_take_base(c, h)) {
    c->stream_mode.delta = ydc_context::Stream::DeltaBase{};
    return rc;
  }
  return YDC_OK;
}

int ydc_stream_delta(ydc_context* c, void* out, size_t cap, size_t* out_bytes) {
  if (!c || !out_bytes) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = delta_mode_check(c, "ydc_stream_delta")) return rc;
  if (!c->stream_mode.delta.on) return fail(c, YDC_ERR_NO_BASE, "ydc_stream_delta: the stream has no base");
  if (int rc = delta_settle(c, "ydc_stream_delta")) return rc;
  return stream_delta(c, out, cap, out_bytes);
}

int ydc_stream_delta_apply(ydc_context* c, const void* blob, size_t bytes) {
  if (!c || !blob) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = delta_mode_check(c, "ydc_stream_delta_apply")) return rc;
  // Everything that can be wrong with the bytes, before anything of the context is looked at.
  delta::View v{};
  if (const char* why = delta::validate(blob, bytes, &v)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_delta_apply: %s", why);
  if (c->stream_mode.inspect.on)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "ydc_stream_delta_apply: inspection is on (a delta carries no inspection "
                "records: ydc_stream_delta_apply_inspected takes it with its sidecar)");
  if (int rc = delta_settle(c, "ydc_stream_delta_apply")) return rc;
  return stream_delta_apply(c, "ydc_stream_delta_apply", v, nullptr);
}

int ydc_stream_delta_stop(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (int rc = delta_mode_check(c, "ydc_stream_delta_stop")) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  auto& b = c->stream_mode.delta;
  DevBuf<uint8_t> keep = std::move(b.apply);  // (a standby's scratch is no base)
  b = ydc_context::Stream::DeltaBase{};
  b.apply = std::move(keep);
  return YDC_OK;
}

// ---- inspection sidecars (stream_inspect_delta.h, stream_inspect_delta_codec.h) ----

// The identity of the context's state as a sidecar names it (the stream at rest: delta_settle).
static int inspect_identity(ydc_context* c, insd::Header* h) {
  auto& sm = c->stream_mode;
  snap::Header sh;
  snap_describe(c, &sh);
  LeaseState lst{};
  HIP_TRY(c, hipMemcpy(&lst, sm.ls, sizeof lst, hipMemcpyDeviceToHost));
  if (lst.n_leases != sh.n_leases)
    return fail(c, YDC_ERR_NOT_CONVERGED, "lease table: |L| %u on the device, %u on the host", lst.n_leases, sh.n_leases);
  h->stamp = delta_stamp(c, sh);
  h->next_id = lst.next_id;
  h->last_now = sh.last_now;
  h->lease_tick = sh.lease_tick;
  h->n_leases = sh.n_leases;
  h->n_servants = sh.n_servants;
  return YDC_OK;
}

static bool inspect_same_state(const insd::Header& a, const insd::Header& b) {
  return a.stamp == b.stamp && a.next_id == b.next_id && a.last_now == b.last_now && a.lease_tick == b.lease_tick &&
         a.n_leases == b.n_leases && a.n_servants == b.n_servants;
}

// The state a delta results in, as a sidecar names it.
static insd::Header inspect_result_of(const delta::Header& d) {
  insd::Header h{};
  h.stamp = d.stamp, h.next_id = d.next_id, h.last_now = d.last_now, h.lease_tick = d.lease_tick;
  h.n_leases = d.n_leases, h.n_servants = d.n_servants;
  return h;
}

int ydc_stream_delta_inspect(ydc_context* c, const void* delta_blob, size_t delta_bytes, void* out, size_t cap,
                             size_t* out_bytes) {
  if (!c || !out_bytes) return YDC_ERR_INVALID_ARGUMENT;
  const char* const who = "ydc_stream_delta_inspect";
  if (int rc = delta_mode_check(c, who)) return rc;
  auto& sm = c->stream_mode;
  if (!sm.inspect.on) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the stream has no inspection", who);
  delta::View dv{};
  if (delta_blob)
    if (const char* why = delta::validate(delta_blob, delta_bytes, &dv)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: %s", who, why);
  if (int rc = delta_settle(c, who)) return rc;
  if (int rc = inspect_fit(c, sm.last_now == INT64_MIN ? 0 : sm.last_now)) return rc;
  insd::Header now{};
  if (int rc = inspect_identity(c, &now)) return rc;
  if (delta_blob && !inspect_same_state(inspect_result_of(dv.h), now))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the delta's result (tick %u, next_id %llu, |L| %u) is not this context's state "
                "(tick %u, next_id %llu, |L| %u): the sidecar is taken before the next tick", who, dv.h.lease_tick,
                (unsigned long long)dv.h.next_id, dv.h.n_leases, now.lease_tick, (unsigned long long)now.next_id, now.n_leases);
  const uint32_t S = now.n_servants, n = delta_blob ? dv.h.n_ins : now.n_leases;
  insd::Header h = insd::describe(delta_blob ? insd::kDelta : insd::kFull, S, n);
  h.stamp = now.stamp, h.next_id = now.next_id, h.last_now = now.last_now, h.lease_tick = now.lease_tick;
  h.n_leases = now.n_leases, h.epoch = sm.inspect.epoch;
  *out_bytes = (size_t)h.total_bytes;
  if (cap < h.total_bytes) return fail(c, YDC_ERR_CAPACITY, "a sidecar of %llu bytes > cap %zu", (unsigned long long)h.total_bytes, cap);
  if (!out) return YDC_ERR_INVALID_ARGUMENT;
  // The records' columns on the host, in id order.
  std::vector<uint64_t> id(n);
  std::vector<int64_t> started(n);
  std::vector<uint32_t> env(n), ip(n);
  std::vector<uint8_t> pre(n);
  if (delta_blob && n) {
    // ids | started_at | env_id | requestor_ip | prefetch | the count of misses
    std::memcpy(id.data(), dv.ins_id, (size_t)n * 8);
    const size_t o_cnt = ((size_t)n * 25 + 3) & ~(size_t)3;
    HIP_TRY(c, sm.inspect.pack.reserve(o_cnt + 4));
    uint8_t* d = sm.inspect.pack.p;
    const InspectRecords recs{(int64_t*)(d + (size_t)n * 8), (uint32_t*)(d + (size_t)n * 16), (uint32_t*)(d + (size_t)n * 20),
                              d + (size_t)n * 24};
    HIP_TRY(c, hipMemcpyAsync(d, id.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_cnt, 0, 4, c->stream));
    YDC_LAUNCH(c, "k_inspect_gather", k_inspect_gather, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, sm.lt, sm.ls,
               sm.d_insp_rec.p, sm.d_insp_pre.p, (const unsigned long long*)d, n, recs, (uint32_t*)(d + o_cnt));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // The four columns and the count behind them, in one copy.
    std::vector<uint8_t> back(o_cnt + 4 - (size_t)n * 8);
    HIP_TRY(c, hipMemcpy(back.data(), d + (size_t)n * 8, back.size(), hipMemcpyDeviceToHost));
    uint32_t missing = 0;
    std::memcpy(&missing, back.data() + back.size() - 4, 4);
    if (missing) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: %u of the delta's %u inserted ids are no lease", who, missing, n);
    std::memcpy(started.data(), back.data(), (size_t)n * 8);
    std::memcpy(env.data(), back.data() + (size_t)n * 8, (size_t)n * 4);
    std::memcpy(ip.data(), back.data() + (size_t)n * 12, (size_t)n * 4);
    std::memcpy(pre.data(), back.data() + (size_t)n * 16, n);
  } else if (n) {
    uint32_t got = 0;
    if (int rc = ydc_stream_inspect_tasks(c, id.data(), nullptr, nullptr, nullptr, started.data(), env.data(), ip.data(),
                                          pre.data(), n, &got))
      return rc;
    if (got != n) return fail(c, YDC_ERR_NOT_CONVERGED, "%s: %u records for |L| %u", who, got, n);
  }
  std::vector<int64_t> disc(S);
  std::vector<uint64_t> ever(S);
  if (S) {
    HIP_TRY(c, hipMemcpy(disc.data(), sm.inspect.disc.p, (size_t)S * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(ever.data(), sm.inspect.ever.p, (size_t)S * 8, hipMemcpyDeviceToHost));
  }
  std::vector<uint8_t> blob;
  insd::build(h, insd::Columns{id.data(), started.data(), env.data(), ip.data(), pre.data(), disc.data(), ever.data()}, &blob);
  std::memcpy(out, blob.data(), blob.size());
  return YDC_OK;
}

int ydc_stream_inspect_restore(ydc_context* c, const void* side, size_t bytes) {
  if (!c || !side) return YDC_ERR_INVALID_ARGUMENT;
  const char* const who = "ydc_stream_inspect_restore";
  if (int rc = delta_mode_check(c, who)) return rc;
  // Everything that can be wrong with the bytes, before anything of the context is looked at.
  insd::View v{};
  if (const char* why = insd::validate(side, bytes, &v)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: %s", who, why);
  if (v.h.kind != insd::kFull) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: a delta's sidecar (ydc_stream_delta_apply_inspected takes it)", who);
  if (int rc = delta_settle(c, who)) return rc;
  auto& sm = c->stream_mode;
  insd::Header now{};
  if (int rc = inspect_identity(c, &now)) return rc;
  if (!inspect_same_state(v.h, now))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the sidecar's state (tick %u, next_id %llu, |L| %u, %u servants) is not this "
                "context's (tick %u, next_id %llu, |L| %u, %u servants)", who, v.h.lease_tick, (unsigned long long)v.h.next_id,
                v.h.n_leases, v.h.n_servants, now.lease_tick, (unsigned long long)now.next_id, now.n_leases, now.n_servants);
  const uint32_t n = v.h.n, S = v.h.n_servants;  // (n == |L|: validate)
  // Every id is a live lease (read-only). The ids ascend, so n distinct leases of |L| == n are all of L.
  DevBuf<unsigned long long> d_id;
  DevBuf<int64_t> d_at;
  DevBuf<uint32_t> d_slot, d_env, d_ip, d_miss;
  DevBuf<uint8_t> d_pre;
  const size_t nn = std::max(n, 1u);
  HIP_TRY(c, d_id.reserve(nn));
  HIP_TRY(c, d_slot.reserve(nn));
  HIP_TRY(c, d_at.reserve(nn));
  HIP_TRY(c, d_env.reserve(nn));
  HIP_TRY(c, d_ip.reserve(nn));
  HIP_TRY(c, d_pre.reserve(nn));
  HIP_TRY(c, d_miss.reserve(1));
  if (n) {
    HIP_TRY(c, hipMemcpy(d_id.p, v.id, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_at.p, v.started_at, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_env.p, v.env_id, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_ip.p, v.requestor_ip, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_pre.p, v.prefetch, n, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(d_miss.p, 0, 4));
    YDC_LAUNCH(c, "k_inspect_find", k_inspect_find, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, sm.lt, sm.ls, d_id.p, n,
               d_slot.p, d_miss.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t missing = 0;
    HIP_TRY(c, hipMemcpy(&missing, d_miss.p, 4, hipMemcpyDeviceToHost));
    if (missing) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: %u of %u ids are no lease", who, missing, n);
  }
  // Room for everything, still before the first write into the context's state.
  const size_t slots = (size_t)sm.lt.mask + 1;
  DevBuf<int64_t> disc;
  DevBuf<unsigned long long> ever;
  DevBuf<uint4> rec;
  DevBuf<uint8_t> pre;
  const bool fresh = !sm.inspect.on;
  if (fresh) {
    HIP_TRY(c, disc.reserve((size_t)S + S / 2 + 1024));
    HIP_TRY(c, ever.reserve((size_t)S + S / 2 + 1024));
    HIP_TRY(c, rec.reserve(slots));
    HIP_TRY(c, pre.reserve(slots));
  } else if (sm.inspect.disc.cap < S || sm.inspect.ever.cap < S) {
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the inspection columns hold %zu rows, %u servants", who, sm.inspect.disc.cap, S);
  }
  // From here on the context is written.
  if (sm.usage.on) sm.usage.fresh += n;  // (the records may name requestors its table has not met)
  if (fresh) {
    sm.inspect.disc = std::move(disc);
    sm.inspect.ever = std::move(ever);
    sm.d_insp_rec = std::move(rec);
    sm.d_insp_pre = std::move(pre);
    YDC_LAUNCH(c, "k_inspect_fill", k_inspect_fill, dim3(ceil_div((uint32_t)slots, 256)), dim3(256), 0, c->stream,
               sm.d_insp_rec.p, sm.d_insp_pre.p, (uint32_t)slots);
    HIP_TRY(c, hipGetLastError());
  }
  if (S) {
    HIP_TRY(c, hipMemcpy(sm.inspect.disc.p, v.discovered_at, (size_t)S * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(sm.inspect.ever.p, v.ever_assigned, (size_t)S * 8, hipMemcpyHostToDevice));
  }
  if (n) {
    YDC_LAUNCH(c, "k_inspect_file", k_inspect_file, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, d_slot.p, n,
               (uint32_t)slots, d_at.p, d_env.p, d_ip.p, d_pre.p, sm.d_insp_rec.p, sm.d_insp_pre.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  sm.inspect.n = S;
  sm.inspect.on = true;
  sm.inspect.epoch = v.h.epoch;
  sm.stale = true;  // (the step's granting pass changes, and it holds the columns' addresses: captured again)
  return YDC_OK;
}

int ydc_stream_delta_apply_inspected(ydc_context* c, const void* blob, size_t bytes, const void* side, size_t side_bytes) {
  if (!c || !blob || !side) return YDC_ERR_INVALID_ARGUMENT;
  const char* const who = "ydc_stream_delta_apply_inspected";
  if (int rc = delta_mode_check(c, who)) return rc;
  // Everything that can be wrong with the bytes, and with the two blobs as a pair, before anything of the
  // context is looked at.
  delta::View v{};
  insd::View sv{};
  if (const char* why = delta::validate(blob, bytes, &v)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the delta: %s", who, why);
  if (const char* why = insd::validate(side, side_bytes, &sv)) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the sidecar: %s", who, why);
  if (sv.h.kind != insd::kDelta) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: a full sidecar (ydc_stream_inspect_restore takes it)", who);
  if (!inspect_same_state(sv.h, inspect_result_of(v.h)))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the sidecar describes another state than the delta results in", who);
  if (sv.h.n != v.h.n_ins || (sv.h.n && std::memcmp(sv.id, v.ins_id, (size_t)sv.h.n * 8)))
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the sidecar's ids are not the delta's inserted ones", who);
  const auto& in = c->stream_mode.inspect;
  if (!in.on) return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the stream has no inspection (ydc_stream_delta_apply is the call)", who);
  if (sv.h.epoch != in.epoch)
    return fail(c, YDC_ERR_INVALID_ARGUMENT, "%s: the sidecar's inspection epoch %llu is not this context's %llu: records were "
                "rewritten on the primary, take a new base", who, (unsigned long long)sv.h.epoch, (unsigned long long)in.epoch);
  if (int rc = delta_settle(c, who)) return rc;
  return stream_delta_apply(c, who, v, &sv);
}

}  // extern "C"

extern "C" {

int ydc_synchronize(ydc_context* c) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  join_lanes(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return YDC_OK;
}

// For the tests (not declared in the header): batches placed so far, how many of the pipelined
// ones were enqueued on the second lane, and how many ydc_dispatch_wait had to place again.
int ydc_debug_pipeline(ydc_context* c, uint64_t* out_batches, uint64_t* out_on_second_lane, uint64_t* out_misses) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  if (out_batches) *out_batches = c->pipeline_batches;
  if (out_on_second_lane) *out_on_second_lane = c->lane1_batches;
  if (out_misses) *out_misses = c->pipeline_misses;
  return YDC_OK;
}

int ydc_set_profiling(ydc_context* c, int on) {
  if (!c) return YDC_ERR_INVALID_ARGUMENT;
  join_lanes(c);
  c->profiling = on != 0;
  return YDC_OK;
}

const char* ydc_kernel_profile(const ydc_context* c) {
  return c ? c->kprofile_json.c_str() : "{}";
}

#ifdef YDC_PHASE_PROBE
// Measurement builds only (`make probe`): the matching kernel's phase stamps, kProbeSlots per chunk.
int ydc_debug_phase_probe(unsigned long long* out, size_t n_words, int clear) {
  const size_t all = (size_t)kProbeChunks * kProbeSlots;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(ydc_phase_probe), std::min(n_words, all) * 8) != hipSuccess)
    return YDC_ERR_HIP;
  if (clear) {
    std::vector<unsigned long long> z(all, 0);
    if (hipMemcpyToSymbol(HIP_SYMBOL(ydc_phase_probe), z.data(), all * 8) != hipSuccess) return YDC_ERR_HIP;
  }
  return YDC_OK;
}
#endif

int ydc_get_stats(const ydc_context* c, ydc_stats* out) {
  if (!c || !out) return YDC_ERR_INVALID_ARGUMENT;
  *out = c->stats;
  out->tick_resident_calls = (uint32_t)c->tick_resident;
  out->tick_launched_calls = (uint32_t)c->tick_launches;
  out->pipeline_batches = (uint32_t)c->pipeline_batches;
  return YDC_OK;
}

}  // extern "C"
