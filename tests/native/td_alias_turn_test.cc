// tests/native/td_alias_turn_test.cc — one turn of the host class GpuTaskDispatcher in which parked
// waiters are renumbered because a requestor alias appears, while new requests arrive. Built
// against the CPU stand-in of the device API (ydc_stub.cc) under ASan + UBSan and under TSan
// (`make aliasturn aliasturn_tsan`), no GPU.
//
// A requestor address becomes an alias when a servant registers whose location has several ':' and
// the address is one of the location's shorter prefixes ("[fe80" for "[fe80:1]:8335",
// task_dispatcher.cc:66-69). The first lookup of such an address after the registration creates the
// alias and moves registry_epoch_, which renumbers the (digest, min_version, host) triples
// (Pending::sig). UnsafeDrainQueue must not keep a number from before that.
//
// The interleaving is made, not hoped for: Options::clock is a function, and the dispatcher reads
// it under its lock (KeepServantAlive: first thing inside its Section; OnExpirationTimer: once
// before the lock and again inside the turn it serves on the way out). The test's clock blocks ONE
// thread at its n-th reading; while it stands there holding the lock, the other threads queue their
// calls; opening the gate lets the holder's ~Section serve the parked requests and all arrivals.
//
//   td_alias_turn_test [out dir] [cases, e.g. AB]
//
// Every case runs with the op log on and writes <out dir>/alias_turn_<case>.json in the form of
// td_linearize.cc (log, final DumpInternals, every thread's calls with their answers and
// intervals): tests/td_scenarios.py:verify_linearizable replays it through the reference class.
// Prints TD-ALIAS-TURN-OK and exits 0 when every case's own checks hold.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gpu_task_dispatcher.h"

using namespace ydc;
using namespace std::literals;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

namespace {
using Clk = std::chrono::steady_clock;
long long WallNs() { return std::chrono::duration_cast<std::chrono::nanoseconds>(Clk::now().time_since_epoch()).count(); }

// The injected clock. Arm(n), called by a thread for itself: that thread's n-th reading from now
// on blocks until Open(). Everybody else reads through.
class GateClock {
 public:
  GpuTaskDispatcher::Clock::time_point Read() {
    {
      std::unique_lock lk(mu_);
      if (block_at_ != 0 && std::this_thread::get_id() == who_ && ++calls_ == block_at_) {
        blocked_.store(true);
        cv_.wait(lk, [this] { return open_; });
      }
    }
    return GpuTaskDispatcher::Clock::time_point(std::chrono::nanoseconds(now_ns_.load()));
  }
  void Arm(int nth) {
    std::scoped_lock _(mu_);
    who_ = std::this_thread::get_id();
    block_at_ = nth;
    calls_ = 0;
    open_ = false;
  }
  void Open() {
    std::scoped_lock _(mu_);
    open_ = true;
    block_at_ = 0;
    blocked_.store(false);
    cv_.notify_all();
  }
  // The armed thread stands in the gate (it holds the dispatcher's lock there).
  void AwaitBlocked() {
    const auto give_up = Clk::now() + 30s;
    while (!blocked_.load()) {
      CHECK(Clk::now() < give_up);
      std::this_thread::sleep_for(1ms);
    }
  }
  void Advance(std::chrono::milliseconds d) { now_ns_.fetch_add(std::chrono::nanoseconds(d).count()); }

 private:
  std::atomic<std::int64_t> now_ns_{5'000'000'000};  // (whole milliseconds: the reference's replay clock)
  std::mutex mu_;
  std::condition_variable cv_;
  std::thread::id who_;
  int block_at_ = 0, calls_ = 0;
  bool open_ = true;
  std::atomic<bool> blocked_{false};
};

struct Op {
  int kind;  // 0 wait, 1 free
  int st;    // 0 granted, 1 EnvironmentNotFound, 2 Timeout
  unsigned long long id;
  std::string loc;
  long long t0, t1;
};

// One thread's calls in program order.
struct Caller {
  std::string ip;  // empty and !has_ip: the thread only frees
  bool has_ip = false;
  std::vector<Op> ops;
};

ServantPersonality Servant(const std::string& loc, std::size_t cap, const std::string& digest) {
  ServantPersonality s;
  s.version = 20;
  s.observed_location = s.reported_location = loc;
  s.environments = {digest};
  s.num_processors = 64;
  s.current_load = 0;
  s.max_tasks = cap;
  s.memory_available_in_bytes = 50ull << 30;
  s.priority = kServantPriorityUser;
  return s;
}

constexpr auto kNoWait = 0ns;
constexpr auto kLong = std::chrono::nanoseconds(3600s);

struct Case {
  GateClock clk;
  std::unique_ptr<GpuTaskDispatcher> td;
  std::deque<Caller> callers;  // (addresses stay put)
  std::atomic<int> about_to_call{0};
  std::vector<std::thread> threads;

  Case() {
    GpuTaskDispatcher::Options opt;
    opt.start_expiration_timer = false;
    opt.clock = [this] { return clk.Read(); };
    td = std::make_unique<GpuTaskDispatcher>(opt);
    CHECK(td->device_status() == 0);
    td->EnableOpLog(true);
  }
  Caller* NewCaller(const char* ip) {
    callers.emplace_back();
    if (ip) {
      callers.back().ip = ip;
      callers.back().has_ip = true;
    }
    return &callers.back();
  }
  // (returns the index of the call in c->ops)
  std::size_t Wait(Caller* c, const std::string& digest, std::uint32_t min_version, std::chrono::nanoseconds wait) {
    TaskPersonality t{c->ip, min_version, digest};
    Op op{0, 0, 0, "", WallNs(), 0};
    const auto r = td->WaitForStartingNewTask(t, 60s, td->Now() + wait, false);
    op.t1 = WallNs();
    CHECK(r.device_error == 0);
    op.st = r.ok ? 0 : r.status == WaitStatus::EnvironmentNotFound ? 1 : 2;
    if (r.ok) {
      op.id = r->task_id;
      op.loc = r->servant_location;
    }
    c->ops.push_back(op);
    return c->ops.size() - 1;
  }
  void Free(Caller* c, unsigned long long id) {
    Op op{1, 0, id, "", WallNs(), 0};
    td->FreeTask(id);
    op.t1 = WallNs();
    c->ops.push_back(op);
  }
  // A waiter of its own thread, parked by the time this returns: its first attempt has been placed
  // (HostStats::requests counts placed requests) and it is parked in the same critical section.
  Caller* ParkWaiter(const char* ip, const std::string& digest, std::uint32_t min_version = 0) {
    const std::uint64_t before = td->host_stats().requests;
    Caller* c = NewCaller(ip);
    threads.emplace_back([this, c, digest, min_version] { Wait(c, digest, min_version, kLong); });
    const auto give_up = Clk::now() + 30s;
    while (td->host_stats().requests == before) {
      CHECK(Clk::now() < give_up);
      std::this_thread::sleep_for(1ms);
    }
    CHECK(c->ops.empty());  // (it has not returned: it waits)
    return c;
  }
  // A thread that stands in the gate inside `call`, at its nth reading of the clock, holding the lock.
  template <class F>
  void GatedCall(int nth, F call) {
    threads.emplace_back([this, nth, call] {
      clk.Arm(nth);
      call();
    });
    clk.AwaitBlocked();
  }
  // A call that queues up behind the gate.
  template <class F>
  void Queued(F call) {
    ++expected_queued;
    threads.emplace_back([this, call] {
      about_to_call.fetch_add(1);
      call();
    });
  }
  int expected_queued = 0;
  // All queued calls are on their way (each bumped the counter just before calling), plus the time
  // it takes a thread to get from there into the queue; then the gate opens and everybody returns
  // except the waiters that are still parked.
  void OpenGate() {
    const auto give_up = Clk::now() + 30s;
    while (about_to_call.load() != expected_queued) {
      CHECK(Clk::now() < give_up);
      std::this_thread::sleep_for(1ms);
    }
    std::this_thread::sleep_for(150ms);
    clk.Open();
  }
  void JoinAll() {
    for (auto& t : threads) t.join();
    threads.clear();
  }
  // The parked waiters' deadlines pass: they return Timeout (polling the injected clock).
  void LetWaitersTimeOut() { clk.Advance(std::chrono::hours(2)); }

  static void JsonStr(std::FILE* f, const std::string& s) {
    std::fputc('"', f);
    for (char c : s) {
      if (c == '"' || c == '\\') std::fputc('\\', f);
      std::fputc(c, f);
    }
    std::fputc('"', f);
  }
  void Write(const std::string& path) {
    const std::string log = td->TakeOpLog();
    const std::string dump = td->DumpInternals();
    std::FILE* f = std::fopen(path.c_str(), "w");
    CHECK(f != nullptr);
    std::fprintf(f, "{\"dump\": %s,\n\"threads\": [", dump.c_str());
    bool first_thread = true;
    for (const Caller& c : callers) {
      std::fprintf(f, "%s{\"ip\": ", first_thread ? "" : ",\n");
      first_thread = false;
      if (c.has_ip) JsonStr(f, c.ip); else std::fputs("null", f);
      std::fputs(", \"ops\": [", f);
      bool first = true;
      for (const Op& op : c.ops) {
        std::fputs(first ? "" : ", ", f);
        first = false;
        if (op.kind == 0) {
          std::fprintf(f, "[\"wait\", %d, ", op.st);
          if (op.st == 0) {
            std::fprintf(f, "%llu, ", op.id);
            JsonStr(f, op.loc);
          } else {
            std::fputs("null, null", f);
          }
          std::fprintf(f, ", %lld, %lld]", op.t0, op.t1);
        } else {
          std::fprintf(f, "[\"free\", %llu, %lld, %lld]", op.id, op.t0, op.t1);
        }
      }
      std::fputs("]}", f);
    }
    std::fprintf(f, "],\n\"log\": %s}\n", log.c_str());
    std::fclose(f);
  }
};

// A, bounds. One servant with one slot, taken; a waiter from "[fe80" parked on it. Behind the gate
// "[fe80:1]:8335" registers (one free slot), and 24 requests with 24 distinct min_version — 24
// triples, numbered 0..23 — arrive with "do not wait". The parked waiter's address has become an
// alias: renumbering it leaves ONE triple. A turn that keeps the arrivals' old numbers indexes a
// two-entry sig_dead_ with them (heap-buffer-overflow in UnsafeDrainQueue under ASan).
// Returns with the waiter still parked (case D goes on from there).
void RunA(Case& k, Caller* main, Caller** waiter, unsigned long long* held,
          std::chrono::nanoseconds alias_servant_lease) {
  k.td->KeepServantAlive(Servant("10.0.0.1:1", 1, "d"), kLong);
  CHECK(main->ops[k.Wait(main, "d", 0, kNoWait)].st == 0);
  *held = main->ops.back().id;
  *waiter = k.ParkWaiter("[fe80", "d");
  k.GatedCall(1, [&k, alias_servant_lease] { k.td->KeepServantAlive(Servant("[fe80:1]:8335", 1, "d"), alias_servant_lease); });
  std::vector<Caller*> arrivals;
  for (int i = 0; i < 24; ++i) {
    Caller* c = k.NewCaller(("7.7.0." + std::to_string(i)).c_str());
    arrivals.push_back(c);
    k.Queued([&k, c, i] { k.Wait(c, "d", (std::uint32_t)i, kNoWait); });
  }
  k.OpenGate();
  // Join everybody but the waiter: it is threads[0].
  for (std::size_t i = 1; i < k.threads.size(); ++i) k.threads[i].join();
  k.threads.resize(1);
  int granted = 0;
  for (std::size_t i = 0; i != arrivals.size(); ++i) {
    const Caller* c = arrivals[i];
    CHECK(c->ops.size() == 1);
    if (i > 20) {
      CHECK(c->ops[0].st == 1);  // no servant is new enough (version 20): nobody is eligible, :104-108
    } else if (c->ops[0].st == 0) {
      CHECK(c->ops[0].loc == "[fe80:1]:8335");  // the only free slot
      ++granted;
    } else {
      CHECK(c->ops[0].st == 2);
    }
  }
  CHECK(granted == 1);
  CHECK((*waiter)->ops.empty());  // a heartbeat wakes nobody: still parked
  CHECK(k.td->host_stats().alias_renumbered_turns == 1);  // (the turn was the one this file is about)
}

void CaseA(const std::string& out) {
  Case k;
  Caller* main = k.NewCaller("9.9.9.9");
  Caller* w = nullptr;
  unsigned long long held = 0;
  RunA(k, main, &w, &held, kLong);
  k.Free(main, held);
  k.JoinAll();
  k.Write(out);
  CHECK(w->ops.size() == 1 && w->ops[0].st == 0 && w->ops[0].loc == "10.0.0.1:1");
}

// B, a wrong answer without any overflow. Eight waiters of ONE triple are parked from "[fe80" on a
// full pool for digest "d" (eight: the first segment of a retry, cap = 8, so it is flushed before
// the arrivals are looked at). Behind the gate "[fe80:1]:8335" registers, advertising "e" with a
// free slot; one thread frees the held grant (so the turn is a retry: FreeTask of an id nobody
// holds would not do, it returns before the notify_all — task_dispatcher.cc:176-180 — here as in
// the reference), one asks for "e" from "7.7.7.7" with "do not wait".
// The reference grants that request "[fe80:1]:8335". What made the unfixed turn answer Timeout:
// the arrival was numbered first, in the epoch of the registration — triple 0; then renumbering
// the parked requests created the alias "[fe80", the table was cleared and their triple became
// the new 0. The retry's segment granted the freed slot to the first waiter, the other seven came
// back Timeout and marked triple 0 dead; the arrival, still carrying its old 0, was declared a
// known Timeout and never sent.
void CaseB(const std::string& out) {
  Case k;
  Caller* main = k.NewCaller("9.9.9.9");
  k.td->KeepServantAlive(Servant("10.0.0.1:1", 1, "d"), kLong);
  CHECK(main->ops[k.Wait(main, "d", 0, kNoWait)].st == 0);
  const unsigned long long held = main->ops.back().id;
  std::vector<Caller*> waiters;
  for (int i = 0; i < 8; ++i) waiters.push_back(k.ParkWaiter("[fe80", "d"));
  k.GatedCall(1, [&k] { k.td->KeepServantAlive(Servant("[fe80:1]:8335", 1, "e"), kLong); });
  Caller* freer = k.NewCaller(nullptr);
  Caller* asker = k.NewCaller("7.7.7.7");
  k.Queued([&k, freer, held] { k.Free(freer, held); });
  k.Queued([&k, asker] { k.Wait(asker, "e", 0, kNoWait); });
  k.OpenGate();
  for (std::size_t i = 8; i < k.threads.size(); ++i) k.threads[i].join();
  k.threads.resize(8);
  k.LetWaitersTimeOut();
  k.JoinAll();
  k.Write(out);
  CHECK(k.td->host_stats().alias_renumbered_turns == 1);
  CHECK(asker->ops.size() == 1);
  CHECK(asker->ops[0].st == 0 && asker->ops[0].loc == "[fe80:1]:8335");
  int granted = 0;
  for (Caller* w : waiters) {
    CHECK(w->ops.size() == 1);
    granted += w->ops[0].st == 0;
  }
  CHECK(granted == 1 && waiters[0]->ops[0].st == 0);  // the freed slot goes to the first in line
}

// C, more than one alias in a turn. "[fe80:1:2]:8335" answers to "[fe80:1:2]", "[fe80:1" and
// "[fe80" — not to "[". Waiters from both shorter prefixes are parked, interleaved by arrival with
// waiters from plain addresses, so that renumbering creates two aliases, the second after requests
// have already been numbered under the first; the arrivals bring the same addresses again, "[" (a
// near miss), and the full host. Three slots are free in the turn (the freed one, two new ones)
// for eleven requests: who gets them is the reference's say (the replay).
void CaseC(const std::string& out) {
  Case k;
  Caller* main = k.NewCaller("9.9.9.9");
  k.td->KeepServantAlive(Servant("10.0.0.1:1", 1, "d"), kLong);
  CHECK(main->ops[k.Wait(main, "d", 0, kNoWait)].st == 0);
  const unsigned long long held = main->ops.back().id;
  std::vector<Caller*> all;
  const char* parked[] = {"[fe80", "8.8.8.1", "[fe80:1", "8.8.8.2", "[fe80", "[fe80:1"};
  for (const char* ip : parked) all.push_back(k.ParkWaiter(ip, "d"));
  const std::size_t n_parked = all.size();
  k.GatedCall(1, [&k] { k.td->KeepServantAlive(Servant("[fe80:1:2]:8335", 2, "d"), kLong); });
  Caller* freer = k.NewCaller(nullptr);
  k.Queued([&k, freer, held] { k.Free(freer, held); });
  const char* arriving[] = {"[", "[fe80:1", "[fe80", "5.5.5.5", "[fe80:1:2]"};
  for (const char* ip : arriving) {
    Caller* c = k.NewCaller(ip);
    all.push_back(c);
    k.Queued([&k, c] { k.Wait(c, "d", 0, kNoWait); });
  }
  k.OpenGate();
  for (std::size_t i = n_parked; i < k.threads.size(); ++i) k.threads[i].join();
  k.threads.resize(n_parked);
  k.LetWaitersTimeOut();
  k.JoinAll();
  k.Write(out);
  int granted = 0;
  for (Caller* c : all) {
    CHECK(c->ops.size() == 1);
    granted += c->ops[0].st == 0;
  }
  CHECK(granted == 3);
  CHECK(k.td->host_stats().alias_renumbered_turns == 1);  // both aliases came up in ONE turn
}

// D, the alias goes away again. As A, but "[fe80:1]:8335" has a short lease and the "[fe80" waiter
// stays parked. Then the clock moves past that lease and the timer fires. OnExpirationTimer reads
// the clock BEFORE it takes the lock, so it cannot be held at its entry with the lock in hand; its
// second reading is inside the turn it serves on its way out (the retry of the parked waiter, whom
// the tick has woken — after the servant, its shorter prefix and so the alias's reason are gone).
// It is held there; new requests — from the former alias, from the expired host, from plain
// addresses — queue up behind it and are served by the same thread's next turn.
void CaseD(const std::string& out) {
  Case k;
  Caller* main = k.NewCaller("9.9.9.9");
  Caller* w = nullptr;
  unsigned long long held = 0;
  RunA(k, main, &w, &held, 5s);
  k.about_to_call.store(0);
  k.expected_queued = 0;
  k.clk.Advance(10s);
  k.GatedCall(2, [&k] { k.td->OnExpirationTimer(); });
  std::vector<Caller*> arrivals;
  const char* arriving[] = {"[fe80", "[fe80:1]", "7.7.0.1", "7.7.0.2", "[", "10.0.0.1"};
  for (const char* ip : arriving) {
    Caller* c = k.NewCaller(ip);
    arrivals.push_back(c);
    k.Queued([&k, c] { k.Wait(c, "d", 0, kNoWait); });
  }
  k.OpenGate();
  for (std::size_t i = 1; i < k.threads.size(); ++i) k.threads[i].join();
  k.threads.resize(1);
  for (Caller* c : arrivals) CHECK(c->ops.size() == 1 && c->ops[0].st == 2);  // the one slot left is taken
  CHECK(w->ops.empty());
  k.Free(main, held);
  k.JoinAll();
  k.Write(out);
  CHECK(k.td->host_stats().alias_renumbered_turns == 1);  // (case A's turn; the expiry creates none)
  CHECK(w->ops.size() == 1 && w->ops[0].st == 0 && w->ops[0].loc == "10.0.0.1:1");
}
}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const std::string cases = argc > 2 ? argv[2] : "ABCD";
  for (char c : cases) {
    const std::string out = dir + "/alias_turn_" + std::string(1, c) + ".json";
    if (c == 'A') CaseA(out);
    else if (c == 'B') CaseB(out);
    else if (c == 'C') CaseC(out);
    else if (c == 'D') CaseD(out);
    else return 2;
    std::printf("case %c written %s\n", c, out.c_str());
    std::fflush(stdout);
  }
  std::printf("TD-ALIAS-TURN-OK\n");
  return 0;
}
