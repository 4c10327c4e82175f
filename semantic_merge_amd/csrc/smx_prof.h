// smx_prof.h -- the library's last-error string and the per-stage device timers of a merge
// (include/smx.h smx_last_error, smx_set_profiling, smx_stage_times).  Part of the
// smx_compose.hip unit: included once, there.
#pragma once

static thread_local std::string g_err;
static int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int smx_set_error(int code, const char* msg) { return set_err(code, msg ? msg : ""); }

// gsort: the generic plan's sort and window planning; segsort: its segmented sort's
// kernels alone (inside gsort); window_g: the generic window kernel; window: the
// presorted one at the normal capacity, including attempts that fail;
// window_wide: its wide (8192-op) instance, a stage of its own so that a merge's
// failed normal attempt is never averaged into the wide launch's time
enum Stage { ST_PLAN, ST_GSORT, ST_WINDOW, ST_WALK, ST_TABLES, ST_MVPREFIX, ST_EMIT, ST_SEGSORT, ST_WINDOW_G,
             ST_WINDOW_WIDE, ST_SMALL, ST_N };
static const char* kStageNames[ST_N] = {"plan",   "gsort",    "window", "walk",    "tables",
                                        "mvprefix", "emit", "segsort", "window_g", "window_wide", "small"};
static std::mutex g_prof_mu;
static int g_prof = 0;
static u32 g_prof_mask = ~0u;  // the stages timed while profiling is on (smx_set_profiling_stages)
static double g_stage_ms[ST_N];
static int64_t g_stage_calls[ST_N];

// Stage events are recorded on the call's stream and only resolved when the
// caller asks for the times (smx_stage_times), so profiling adds no host sync.
struct PendingEv {
  int stage;
  hipEvent_t a, b;
};
static std::vector<PendingEv> g_pending;

// Timing events are reused: creating and destroying a dozen per merge sat on the host
// path between one merge's sync and the next merge's first launch.  (g_prof_mu guards
// the pool.)
static std::vector<hipEvent_t> g_ev_pool;
static hipEvent_t ev_acquire() {
  {
    std::lock_guard<std::mutex> g(g_prof_mu);
    if (!g_ev_pool.empty()) {
      hipEvent_t e = g_ev_pool.back();
      g_ev_pool.pop_back();
      return e;
    }
  }
  hipEvent_t e = nullptr;
  // timing only (read after the caller's sync): no system-scope fence, whose cache
  // write-back and invalidate at every record cost the timed merges ~40 us on config 3
  // (2.380 ms with the stage timers on against 2.342 ms off, measured in round 5)
  (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return e;
}
static void ev_release_locked(hipEvent_t e) {  // (caller holds g_prof_mu)
  if (e) g_ev_pool.push_back(e);
}

struct StageTimer {
  hipStream_t st;
  bool on;
  u32 mask = ~0u;
  hipEvent_t open[ST_N];
  std::vector<PendingEv> done;
  bool is_open[ST_N] = {};
  StageTimer(hipStream_t s, bool enabled) : st(s), on(enabled) {
    if (on) {
      std::lock_guard<std::mutex> g(g_prof_mu);
      mask = g_prof_mask;
    }
  }
  void begin(int i) {
    if (!on || !((mask >> i) & 1u)) return;
    if (!is_open[i]) open[i] = ev_acquire();  // (a restarted stage re-records its open event)
    (void)hipEventRecord(open[i], st);
    is_open[i] = true;
  }
  void end(int i) {
    if (!on || !is_open[i]) return;
    hipEvent_t b = ev_acquire();
    (void)hipEventRecord(b, st);
    done.push_back({i, open[i], b});
    is_open[i] = false;
  }
  void flush() {
    if (!on) return;
    std::lock_guard<std::mutex> g(g_prof_mu);
    for (auto& p : done) g_pending.push_back(p);
    done.clear();
  }
  ~StageTimer() {  // an error path left events unpublished: back to the pool
    if (done.empty() && !std::any_of(is_open, is_open + ST_N, [](bool b) { return b; })) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return;  // a capturing stream must not be synchronized: these events are left to leak
    }
    (void)hipStreamSynchronize(st);  // (recorded events may still be pending)
    std::lock_guard<std::mutex> g(g_prof_mu);
    for (auto& p : done) {
      ev_release_locked(p.a);
      ev_release_locked(p.b);
    }
    for (int i = 0; i < ST_N; ++i)
      if (is_open[i]) ev_release_locked(open[i]);
  }
};

static void resolve_pending_locked() {
  for (auto& p : g_pending) {
    (void)hipEventSynchronize(p.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p.a, p.b);
    g_stage_ms[p.stage] += ms;
    g_stage_calls[p.stage] += 1;
    ev_release_locked(p.a);
    ev_release_locked(p.b);
  }
  g_pending.clear();
}

static int profiling_on() {
  std::lock_guard<std::mutex> g(g_prof_mu);
  return g_prof;
}

extern "C" int smx_set_profiling(int enabled) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof = enabled;
  return SMX_OK;
}

extern "C" int smx_set_profiling_stages(uint32_t mask) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof_mask = mask;
  return SMX_OK;
}

extern "C" int smx_reset_stage_times(void) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  resolve_pending_locked();
  for (int i = 0; i < ST_N; ++i) {
    g_stage_ms[i] = 0;
    g_stage_calls[i] = 0;
  }
  return SMX_OK;
}

extern "C" int smx_stage_times(double* ms, int64_t* calls, int cap) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  resolve_pending_locked();
  for (int i = 0; i < ST_N && i < cap; ++i) {
    if (ms) ms[i] = g_stage_ms[i];
    if (calls) calls[i] = g_stage_calls[i];
  }
  return ST_N;
}

extern "C" const char* smx_stage_name(int i) { return (i >= 0 && i < ST_N) ? kStageNames[i] : ""; }

extern "C" const char* smx_last_error(void) { return g_err.c_str(); }
