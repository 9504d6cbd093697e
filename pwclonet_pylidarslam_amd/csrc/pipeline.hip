// The throughput pipelines' stream set (include/pwclo_ops.h, section 0b).
//
// The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues and serialises streams that share one.
// Which queue a stream gets is decided by the order in which the process's streams are created / first used, so a
// pipeline whose streams are first used one by one, between the side and capture streams of its slots' graph captures,
// ends up with two of them on one queue.  Here all streams of a set are created back to back and each gets one trivial
// launch, in order, inside the create call: whether the runtime binds at creation or at first use, the set's streams
// are bound consecutively, with nothing of the process in between.
//
// Two additions ("priority classes and the probe"):
// * layouts: the streams of a set may be created in another priority class (hipStreamCreateWithPriority), all of them
//   or the ones past the first hw_queues - 1.  Only the create call differs.
// * the probe: every set measures, once, inside its create call, how many of its streams run side by side: one small
//   ALU-only workgroup per stream, launched back to back, each stamping its start and end on the constant clock.
#include <mutex>

#include "common.hpp"

namespace pwclo {

__global__ void stream_set_touch_kernel() {}

// The probe's launch: one workgroup of 64 threads that runs `trips` rounds of a dependent integer chain (no memory
// traffic, nothing it waits for: it ends by itself after trips rounds) between two reads of the constant 100 MHz clock.
// stamp[3 * at + {0, 1, 2}] = start, end, the chain's value (what keeps the chain alive), written by thread 0.
constexpr int PROBE_WORDS = 3;
constexpr unsigned PROBE_CAL_TRIPS = 1u << 14;      // the calibration launch
constexpr unsigned PROBE_MIN_TRIPS = 1u << 10;
constexpr unsigned PROBE_MAX_TRIPS = 1u << 22;      // whatever the calibration measured, a launch ends after this many
constexpr long long PROBE_TARGET_TICKS = 50000;     // 0.5 ms of the 100 MHz clock
constexpr long long NS_PER_TICK = 10;

__global__ void __launch_bounds__(64) stream_set_probe_kernel(unsigned long long *stamp, int at, unsigned trips) {
  const unsigned long long t0 = (unsigned long long)wall_clock64();
  unsigned x = threadIdx.x + 1u;
  for (unsigned i = 0; i < trips; ++i) {
    x = x * 1664525u + 1013904223u;
    asm volatile("" : "+v"(x));                     // one round per trip: not folded, not vectorised away
  }
  const unsigned long long t1 = (unsigned long long)wall_clock64();
  if (threadIdx.x == 0) {
    stamp[PROBE_WORDS * at + 0] = t0;
    stamp[PROBE_WORDS * at + 1] = t1;
    stamp[PROBE_WORDS * at + 2] = x;
  }
}

struct StreamSet {
  long long id;
  int n;
  int layout;                                 // the layout in effect (0 where the device has one priority level)
  int side_by_side;                           // the probe's result, measured once in the create call
  unsigned together;                          // bit i: stream i is one of the side_by_side that ran together
  long long probe_ns;                         // the longest of the probe's launches
  unsigned long long *stamp;                  // device, PROBE_WORDS * PWCLO_STREAM_SET_MAX words
  hipStream_t stream[PWCLO_STREAM_SET_MAX];
  hipEvent_t arrive[PWCLO_STREAM_SET_MAX];   // per stream: the foreign stream's position that stream i waits for
  hipEvent_t done[PWCLO_STREAM_SET_MAX];     // per slot: completion
  bool recorded[PWCLO_STREAM_SET_MAX];
};

// Handles are ids that are never reused: a destroyed handle stays invalid for the life of the process.
static std::mutex g_sets_mutex;
static StreamSet *g_sets[PWCLO_STREAM_SET_LIVE_MAX] = {};
static long long g_next_id = 1;

static StreamSet *find_locked(long long handle) {
  if (handle <= 0) return nullptr;
  for (StreamSet *s : g_sets)
    if (s != nullptr && s->id == handle) return s;
  return nullptr;
}

static int hip_code(hipError_t e) {
  if (e != hipSuccess) (void)hipGetLastError();   // not left behind for an unrelated launch check
  return (int)e;
}

// Frees whatever of `s` exists (null members are skipped); the first failure is returned, the rest is still freed.
static int release(StreamSet *s) {
  int rc = 0;
  for (int i = 0; i < PWCLO_STREAM_SET_MAX; ++i) {
    if (s->arrive[i] != nullptr) { const int e = hip_code(hipEventDestroy(s->arrive[i])); if (rc == 0) rc = e; }
    if (s->done[i] != nullptr) { const int e = hip_code(hipEventDestroy(s->done[i])); if (rc == 0) rc = e; }
  }
  for (int i = 0; i < s->n; ++i)
    if (s->stream[i] != nullptr) { const int e = hip_code(hipStreamDestroy(s->stream[i])); if (rc == 0) rc = e; }
  if (s->stamp != nullptr) { const int e = hip_code(hipFree(s->stamp)); if (rc == 0) rc = e; }
  delete s;
  return rc;
}

// GPU_MAX_HW_QUEUES as the runtime reads it (4 when unset).  Only ever read.
static int hw_queues() {
  const char *e = getenv("GPU_MAX_HW_QUEUES");
  const int q = e != nullptr ? atoi(e) : 0;
  return q > 0 ? q : 4;
}

// The largest group of launches whose intervals overlap pairwise by more than half the longer one's length; among
// groups of equal size the one of the lowest stream indices.  t[PROBE_WORDS * i + {0, 1}] = start, end of launch i.
static int largest_overlap(const unsigned long long *t, int n, unsigned *members) {
  bool pair[PWCLO_STREAM_SET_MAX][PWCLO_STREAM_SET_MAX];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const long long a0 = (long long)t[PROBE_WORDS * i], a1 = (long long)t[PROBE_WORDS * i + 1];
      const long long b0 = (long long)t[PROBE_WORDS * j], b1 = (long long)t[PROBE_WORDS * j + 1];
      const long long both = (a1 < b1 ? a1 : b1) - (a0 > b0 ? a0 : b0);
      const long long longer = (a1 - a0) > (b1 - b0) ? (a1 - a0) : (b1 - b0);
      pair[i][j] = i == j || 2 * both > longer;
    }
  int best = 0;
  unsigned best_mask = 0u;
  for (unsigned mask = 1u; mask < (1u << n); ++mask) {     // n <= 8: every group is looked at, in rising order
    const int size = __builtin_popcount(mask);
    if (size <= best) continue;
    bool all = true;
    for (int i = 0; i < n && all; ++i)
      for (int j = i + 1; j < n && all; ++j)
        if ((mask >> i & 1u) && (mask >> j & 1u)) all = pair[i][j];
    if (all) { best = size; best_mask = mask; }
  }
  *members = best_mask;
  return best;
}

// Calibrates the probe's launch on stream 0 (one launch of PROBE_CAL_TRIPS), then launches it once per stream, back to
// back, waits for each stream and counts.  Fills s->side_by_side, s->together, s->probe_ns.
static hipError_t probe(StreamSet *s) {
  unsigned long long t[PROBE_WORDS * PWCLO_STREAM_SET_MAX] = {};
  hipError_t e = hipMalloc((void **)&s->stamp, sizeof(t));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(stream_set_probe_kernel, dim3(1), dim3(64), 0, s->stream[0], s->stamp, 0, PROBE_CAL_TRIPS);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream[0]);
  if (e == hipSuccess) e = hipMemcpy(t, s->stamp, sizeof(t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  const long long cal = (long long)(t[1] - t[0]);
  long long trips = cal > 0 ? (long long)PROBE_CAL_TRIPS * PROBE_TARGET_TICKS / cal : (long long)PROBE_MAX_TRIPS;
  if (trips < (long long)PROBE_MIN_TRIPS) trips = PROBE_MIN_TRIPS;
  if (trips > (long long)PROBE_MAX_TRIPS) trips = PROBE_MAX_TRIPS;
  for (int i = 0; i < s->n && e == hipSuccess; ++i) {
    hipLaunchKernelGGL(stream_set_probe_kernel, dim3(1), dim3(64), 0, s->stream[i], s->stamp, i, (unsigned)trips);
    e = hipGetLastError();
  }
  // every stream that got a launch is waited for, also after a failure
  for (int i = 0; i < s->n; ++i) {
    const hipError_t w = hipStreamSynchronize(s->stream[i]);
    if (e == hipSuccess) e = w;
  }
  if (e == hipSuccess) e = hipMemcpy(t, s->stamp, sizeof(t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  s->side_by_side = largest_overlap(t, s->n, &s->together);
  s->probe_ns = 0;
  for (int i = 0; i < s->n; ++i) {
    const long long ns = (long long)(t[PROBE_WORDS * i + 1] - t[PROBE_WORDS * i]) * NS_PER_TICK;
    if (ns > s->probe_ns) s->probe_ns = ns;
  }
  return hipSuccess;
}

// One set of n streams in `layout` (a PWCLO_STREAM_LAYOUT_* other than _AUTO), probed, not yet in the table.
static int make_set(int n, int layout, StreamSet **out) {
  *out = nullptr;
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return hip_code(e);
  if (least == greatest) layout = PWCLO_STREAM_LAYOUT_NORMAL;      // one priority level: nothing to choose
  if (layout == PWCLO_STREAM_LAYOUT_MIXED && hw_queues() - 1 >= n) layout = PWCLO_STREAM_LAYOUT_NORMAL;   // all normal
  StreamSet *s = new StreamSet();   // value-initialised: every member null
  s->n = n;
  s->layout = layout;
  // the events first: between the first stream's creation and the last stream's first launch nothing else is made
  for (int i = 0; i < PWCLO_STREAM_SET_MAX && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&s->arrive[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done[i], hipEventDisableTiming);
  }
  const int normal_first = layout == PWCLO_STREAM_LAYOUT_MIXED ? hw_queues() - 1 : 0;
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    const bool normal = layout == PWCLO_STREAM_LAYOUT_NORMAL || i < normal_first;
    if (normal)
      e = hipStreamCreateWithFlags(&s->stream[i], hipStreamNonBlocking);
    else
      e = hipStreamCreateWithPriority(&s->stream[i], hipStreamNonBlocking,
                                      layout == PWCLO_STREAM_LAYOUT_LOW ? least : greatest);
  }
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    hipLaunchKernelGGL(stream_set_touch_kernel, dim3(1), dim3(1), 0, s->stream[i]);
    e = hipGetLastError();
  }
  for (int i = 0; i < n && e == hipSuccess; ++i) e = hipStreamSynchronize(s->stream[i]);
  if (e == hipSuccess) e = probe(s);
  if (e != hipSuccess) {
    const int rc = hip_code(e);
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    (void)release(s);
    return rc;
  }
  *out = s;
  return 0;
}

}  // namespace pwclo

extern "C" {

int pwclo_stream_set_create_ex(int n, int layout, long long *handle) {
  using namespace pwclo;
  if (handle == nullptr) return PWCLO_EINVAL;
  *handle = 0;
  if (n < 1 || n > PWCLO_STREAM_SET_MAX) return PWCLO_EINVAL;
  if (layout < PWCLO_STREAM_LAYOUT_AUTO || layout > PWCLO_STREAM_LAYOUT_MIXED) return PWCLO_EINVAL;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  int at = -1;
  for (int i = 0; i < PWCLO_STREAM_SET_LIVE_MAX && at < 0; ++i)
    if (g_sets[i] == nullptr) at = i;
  if (at < 0) return PWCLO_EINVAL;
  StreamSet *s = nullptr;
  int rc = 0;
  if (layout != PWCLO_STREAM_LAYOUT_AUTO) {
    rc = make_set(n, layout, &s);
  } else {
    // the first layout whose streams all ran side by side; a set that loses is destroyed as _destroy does it (the
    // device waited for first) before the next is made, and if every layout loses the set is a normal one
    static const int order[] = {PWCLO_STREAM_LAYOUT_NORMAL, PWCLO_STREAM_LAYOUT_MIXED, PWCLO_STREAM_LAYOUT_HIGH,
                                PWCLO_STREAM_LAYOUT_LOW, PWCLO_STREAM_LAYOUT_NORMAL};
    for (int k = 0; k < 5; ++k) {
      if (order[k] == PWCLO_STREAM_LAYOUT_MIXED && hw_queues() - 1 >= n) continue;   // no stream past the normal ones
      rc = make_set(n, order[k], &s);
      if (rc != 0) break;
      // the last try, or a device with one priority level (make_set turned the layout into the normal one, which has
      // been tried): this set is the answer
      const bool last = k == 4 || (k > 0 && s->layout == PWCLO_STREAM_LAYOUT_NORMAL);
      if (last || s->side_by_side == n) break;
      rc = hip_code(hipDeviceSynchronize());
      const int rel = release(s);
      s = nullptr;
      if (rc == 0) rc = rel;
      if (rc != 0) break;
    }
  }
  if (rc != 0) return rc;
  s->id = g_next_id++;
  g_sets[at] = s;
  *handle = s->id;
  return 0;
}

int pwclo_stream_set_create(int n, long long *handle) {
  return pwclo_stream_set_create_ex(n, PWCLO_STREAM_LAYOUT_NORMAL, handle);
}

int pwclo_stream_set_concurrency(long long handle, int *side_by_side) {
  using namespace pwclo;
  if (side_by_side == nullptr) return PWCLO_EINVAL;
  *side_by_side = 0;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  const StreamSet *s = find_locked(handle);
  if (s == nullptr) return PWCLO_EINVAL;
  *side_by_side = s->side_by_side;
  return 0;
}

int pwclo_stream_set_probe(long long handle, int *layout, unsigned *together, long long *probe_ns) {
  using namespace pwclo;
  if (layout == nullptr || together == nullptr || probe_ns == nullptr) return PWCLO_EINVAL;
  *layout = 0;
  *together = 0u;
  *probe_ns = 0;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  const StreamSet *s = find_locked(handle);
  if (s == nullptr) return PWCLO_EINVAL;
  *layout = s->layout;
  *together = s->together;
  *probe_ns = s->probe_ns;
  return 0;
}

int pwclo_stream_set_size(long long handle) {
  using namespace pwclo;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  const StreamSet *s = find_locked(handle);
  return s != nullptr ? s->n : -PWCLO_EINVAL;
}

int pwclo_stream_set_stream(long long handle, int i, void **hip_stream) {
  using namespace pwclo;
  if (hip_stream == nullptr) return PWCLO_EINVAL;
  *hip_stream = nullptr;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  const StreamSet *s = find_locked(handle);
  if (s == nullptr || i < 0 || i >= s->n) return PWCLO_EINVAL;
  *hip_stream = (void *)s->stream[i];
  return 0;
}

int pwclo_stream_set_wait_stream(long long handle, int i, void *other_stream) {
  using namespace pwclo;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  StreamSet *s = find_locked(handle);
  if (s == nullptr || i < 0 || i >= s->n) return PWCLO_EINVAL;
  if ((hipStream_t)other_stream == s->stream[i]) return 0;
  hipError_t e = hipEventRecord(s->arrive[i], (hipStream_t)other_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(s->stream[i], s->arrive[i], 0);
  return hip_code(e);
}

int pwclo_stream_set_record(long long handle, int slot, int i) {
  using namespace pwclo;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  StreamSet *s = find_locked(handle);
  if (s == nullptr || slot < 0 || slot >= PWCLO_STREAM_SET_MAX || i < 0 || i >= s->n) return PWCLO_EINVAL;
  const hipError_t e = hipEventRecord(s->done[slot], s->stream[i]);
  if (e == hipSuccess) s->recorded[slot] = true;
  return hip_code(e);
}

int pwclo_stream_set_query(long long handle, int slot) {
  using namespace pwclo;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  StreamSet *s = find_locked(handle);
  if (s == nullptr || slot < 0 || slot >= PWCLO_STREAM_SET_MAX) return -PWCLO_EINVAL;
  if (!s->recorded[slot]) return 1;
  const hipError_t e = hipEventQuery(s->done[slot]);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    return 0;
  }
  return -hip_code(e);
}

int pwclo_stream_set_wait_slot(long long handle, int slot, void *waiting_stream) {
  using namespace pwclo;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  StreamSet *s = find_locked(handle);
  if (s == nullptr || slot < 0 || slot >= PWCLO_STREAM_SET_MAX) return PWCLO_EINVAL;
  if (!s->recorded[slot]) return 0;
  return hip_code(hipStreamWaitEvent((hipStream_t)waiting_stream, s->done[slot], 0));
}

int pwclo_stream_set_synchronize_slot(long long handle, int slot) {
  using namespace pwclo;
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_sets_mutex);
    StreamSet *s = find_locked(handle);
    if (s == nullptr || slot < 0 || slot >= PWCLO_STREAM_SET_MAX) return PWCLO_EINVAL;
    if (!s->recorded[slot]) return 0;
    ev = s->done[slot];
  }
  return hip_code(hipEventSynchronize(ev));   // the host wait is made without the table's lock
}

int pwclo_stream_set_synchronize(long long handle) {
  using namespace pwclo;
  hipStream_t st[PWCLO_STREAM_SET_MAX];
  int n = 0;
  {
    std::lock_guard<std::mutex> lock(g_sets_mutex);
    StreamSet *s = find_locked(handle);
    if (s == nullptr) return PWCLO_EINVAL;
    n = s->n;
    for (int i = 0; i < n; ++i) st[i] = s->stream[i];
  }
  for (int i = 0; i < n; ++i) {
    const hipError_t e = hipStreamSynchronize(st[i]);
    if (e != hipSuccess) return hip_code(e);
  }
  return 0;
}

int pwclo_stream_set_destroy(long long handle) {
  using namespace pwclo;
  StreamSet *s = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_sets_mutex);
    s = find_locked(handle);
    if (s == nullptr) return PWCLO_EINVAL;
    for (StreamSet *&slot : g_sets)
      if (slot == s) slot = nullptr;   // from here on the handle is refused
  }
  // work queued on the set's streams, and work of other streams that waits for the set's events, ends first
  const int rc = hip_code(hipDeviceSynchronize());
  const int rel = release(s);
  return rc != 0 ? rc : rel;
}

}  // extern "C"
