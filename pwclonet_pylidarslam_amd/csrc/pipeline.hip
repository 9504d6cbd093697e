// The throughput pipelines' stream set (include/pwclo_ops.h, section 0b).
//
// The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues and serialises streams that share one.
// Which queue a stream gets is decided by the order in which the process's streams are created / first used, so a
// pipeline whose streams are first used one by one, between the side and capture streams of its slots' graph captures,
// ends up with two of them on one queue.  Here all streams of a set are created back to back and each gets one trivial
// launch, in order, inside the create call: whether the runtime binds at creation or at first use, the set's streams
// are bound consecutively, with nothing of the process in between.
#include <mutex>

#include "common.hpp"

namespace pwclo {

__global__ void stream_set_touch_kernel() {}

struct StreamSet {
  long long id;
  int n;
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
  delete s;
  return rc;
}

}  // namespace pwclo

extern "C" {

int pwclo_stream_set_create(int n, long long *handle) {
  using namespace pwclo;
  if (handle == nullptr) return PWCLO_EINVAL;
  *handle = 0;
  if (n < 1 || n > PWCLO_STREAM_SET_MAX) return PWCLO_EINVAL;
  std::lock_guard<std::mutex> lock(g_sets_mutex);
  int at = -1;
  for (int i = 0; i < PWCLO_STREAM_SET_LIVE_MAX && at < 0; ++i)
    if (g_sets[i] == nullptr) at = i;
  if (at < 0) return PWCLO_EINVAL;
  StreamSet *s = new StreamSet();   // value-initialised: every member null
  s->n = n;
  hipError_t e = hipSuccess;
  // the events first: between the first stream's creation and the last stream's first launch nothing else is made
  for (int i = 0; i < PWCLO_STREAM_SET_MAX && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&s->arrive[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done[i], hipEventDisableTiming);
  }
  for (int i = 0; i < n && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&s->stream[i], hipStreamNonBlocking);
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    hipLaunchKernelGGL(stream_set_touch_kernel, dim3(1), dim3(1), 0, s->stream[i]);
    e = hipGetLastError();
  }
  for (int i = 0; i < n && e == hipSuccess; ++i) e = hipStreamSynchronize(s->stream[i]);
  if (e != hipSuccess) {
    const int rc = hip_code(e);
    (void)release(s);
    return rc;
  }
  s->id = g_next_id++;
  g_sets[at] = s;
  *handle = s->id;
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
