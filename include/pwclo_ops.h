/*
 * pwclo_ops.h -- C ABI of libpwclo_hip.so, the MI355X (gfx950) implementation of the
 * PWCLO-Net point-cloud operator path.
 *
 * Drop-in boundary.  The reference's extension is split into C++ host files that check and
 * allocate torch tensors and then call plain C++ launchers taking raw device pointers and
 * 32-bit sizes.  Those nine launchers are the FFI of this path; section 1 exports them with the
 * reference's exact names, argument order and meaning (extern "C"; the reference declares them
 * at the cited lines inside its .cpp files, so relinking its host files against this library
 * needs only `extern "C"` around those declarations -- see INTEGRATION.md).
 *
 * All pointers are device pointers on the current HIP device.  Tensors are dense, row-major
 * ("contiguous" in the reference's CHECK_CONTIGUOUS sense), float = IEEE binary32, int = int32.
 * Calls enqueue on the stream set by pwclo_set_stream() for the calling host thread (default:
 * the null stream) and return without synchronising -- the reference launches on ATen's current
 * stream the same way (e.g. group_points_gpu.cu:34).  No entry point allocates, frees or
 * synchronises, so every call may be captured into a hipGraph.
 *
 * Errors.  The reference prints and calls exit(-1) when a launch fails (cuda_utils.h:30-39).
 * This library never exits the process: it prints one line to stderr, records the failure in a
 * per-thread sticky status readable through pwclo_last_error(), and skips the launch.  Host
 * bindings must check pwclo_last_error() after a call and raise (ours do).
 *
 * Reference paths below are relative to
 *   /root/reference/slam/models/Pointnet2_PyTorch/pointnet2_ops_lib/pointnet2_ops/_ext-src/src/
 */
#ifndef PWCLO_OPS_H
#define PWCLO_OPS_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 0. library state ------------------------------------------------------------------- */

/* Version of this ABI (bumped on any signature change). */
int pwclo_abi_version(void);

/* Set / get the hipStream_t (passed as void*) used by the calling host thread's launches.
 * Replaces at::cuda::getCurrentCUDAStream() inside the reference launchers. */
void pwclo_set_stream(void *hip_stream);
void *pwclo_get_stream(void);

/* 0 = no error since the last pwclo_clear_error() on this thread, else a hipError_t value or
 * one of the PWCLO_E* codes.  pwclo_last_error_message() returns a static thread-local string. */
int pwclo_last_error(void);
const char *pwclo_last_error_message(void);
void pwclo_clear_error(void);

/* Launch record.  The launch layer of the fused stack kernels, the linear jobs and the register / slab samplers
 * (csrc/common.hpp: launch_grid) notes, per host thread, the kernel it launched last.  pwclo_take_launch() hands that
 * record out and clears it: 1 with name = the instantiation as rocprofv3 prints it, e.g. "cv_a2_kernel<32, 2, 8, 0,
 * false>" (the runtime's symbol of the launched kernel, demangled, without "void pwclo::" and the parameter list;
 * truncated to name_cap - 1 characters) and geometry = {waves per workgroup, grid x, grid y, dynamic LDS bytes};
 * 0, outputs untouched, when the thread has launched nothing through that layer since the last take, or when a call
 * has failed since (a failed call leaves no record).  Either pointer may be NULL.  To learn what ONE call launched,
 * take (and discard) before it and take after it.  Launches that bypass launch_grid are not recorded.
 * pwclo_set_dry_run(1): until switched off, this thread's launch_grid launches are recorded but NOT made, and the
 * launch check that follows them does not ask the runtime -- a wrapper's whole dispatch, argument guards included,
 * runs on a machine without a GPU.  It covers ONLY launches through launch_grid: every other entry point still
 * launches, so switch it on around calls of the recorded kernels alone. */
int pwclo_take_launch(char *name, int name_cap, int *geometry);
void pwclo_set_dry_run(int on);

/* Developer tool: per-workgroup trace of the kernels on the fused forward path.  records: device buffer of
 * `capacity` 32-byte records {u64 t0, t1 (100 MHz constant clock); u32 kernel id, block, blocks in grid, hw id};
 * count: device u32 the kernels bump (zero it first).  records == NULL switches the trace off (the default).
 * Synchronous (writes device symbols); not for use under graph capture. */
void pwclo_trace_enable(void *records, void *count, unsigned capacity);

/* How furthest_point_sampling launches its multi-workgroup kernel for clouds too large for one workgroup (n > 24576):
 * cooperative != 0 (default; PWCLO_FPS_COOP_LAUNCH): hipLaunchCooperativeKernel -- co-residency guaranteed by the
 * runtime, but the device has ONE cooperative queue: such launches on different streams run one after the other;
 * cooperative == 0: plain launch, for a caller that keeps two large-cloud batches in flight and bounds the workgroups in
 * flight itself (<= 256 of this kernel).  Either way a workgroup that waits for its peers beyond the spin bound reports
 * PWCLO_ECOOP_TIMEOUT through pwclo_last_error(); the indices are never silently incomplete.  Process-wide. */
void pwclo_fps_large_cloud_launch(int cooperative);
/* The same kernel's cross-workgroup exchange.  xcd_local != 0 (default; PWCLO_FPS_COOP_XCD_LOCAL): the workgroups of a
 * cloud are drawn from blocks with equal index mod 8, which the dispatcher deals to one XCD; every launch CHECKS that
 * (the workgroups exchange their XCC ids first) and only then posts with plain stores that stay in that XCD's L2, where
 * the peers' L1-bypassing polls find them (2.3 instead of 2.6 us per sample).  If the ids differ, or with xcd_local == 0,
 * the posts are agent-scope stores as before.  Same indices either way.  Process-wide. */
void pwclo_fps_large_cloud_exchange(int xcd_local);

#define PWCLO_EINVAL 10001  /* argument outside what the kernels support (message says which) */
/* Reported by a RUNNING kernel (not at launch): the cooperative large-cloud sampler gave up waiting for a
 * peer workgroup.  Kernels post such codes into a pinned word the library owns; pwclo_last_error() reads it
 * without a HIP call, so it becomes visible once the kernel has run: at the next library call, or when the
 * host calls pwclo_last_error() after synchronising the stream.  The outputs of that call are invalid. */
#define PWCLO_ECOOP_TIMEOUT 10002

/* ---- 0b. the pipelines' stream set (csrc/pipeline.hip) ------------------------------------ */

/* A set of n HIP streams for a pipeline that keeps several captured forwards in flight (graphed.PipelinedForward), plus
 * one completion event per slot.  The runtime serialises streams that share a hardware queue, and which queue a stream gets
 * follows from the order in which the process's streams are created / first used.  pwclo_stream_set_create makes all n
 * streams back to back (hipStreamNonBlocking, normal priority), then one empty launch on each, in order, and waits for
 * those: the set's streams are bound to consecutive hardware queues with no other stream of the process in between.  Then
 * it measures how many of them run side by side (the probe, below).  No CU mask, no change of the queue count.
 *
 * Handles are positive ids that are never reused.  Every function returns 0 on success, PWCLO_EINVAL for an argument it
 * refuses (n outside [1, PWCLO_STREAM_SET_MAX], a stream or slot index out of range, a handle that was never issued or is
 * destroyed, a NULL result pointer, more than PWCLO_STREAM_SET_LIVE_MAX live sets) -- decided before any HIP call, so a
 * refusal never touches the device -- or the hipError_t of the HIP call that failed.  The per-thread sticky status of
 * pwclo_last_error() is not used here.  Streams travel as void* (hipStream_t), like pwclo_set_stream's.  None of these
 * calls may be made while the calling thread captures a graph, except _stream and _size. */
#define PWCLO_STREAM_SET_MAX 8        /* streams per set, and completion slots per set */
#define PWCLO_STREAM_SET_LIVE_MAX 64  /* sets alive at once in a process */
int pwclo_stream_set_create(int n, long long *handle);
/* The same with a choice of the streams' priority class (pwclo_stream_set_create is _NORMAL).  The runtime keeps its
 * hardware queues per priority class, so a stream of another class does not share a queue with the process's normal
 * streams.  _HIGH / _LOW: every stream at the greatest / least priority of hipDeviceGetStreamPriorityRange; _MIXED:
 * streams 0 .. k-1 normal and the rest high, k = GPU_MAX_HW_QUEUES - 1 (4 - 1 when unset; the variable is only read);
 * _AUTO: tries _NORMAL, _MIXED, _HIGH, _LOW in that order and keeps the first set whose probe (below) finds all n
 * streams side by side, a _NORMAL set if none does; a set that loses is destroyed as pwclo_stream_set_destroy does it.
 * Only the create call of a stream differs between layouts.  On a device with one priority level every layout is
 * _NORMAL, and so is _MIXED with n <= k; pwclo_stream_set_probe reports it so.  Any other layout value: PWCLO_EINVAL. */
#define PWCLO_STREAM_LAYOUT_AUTO (-1)
#define PWCLO_STREAM_LAYOUT_NORMAL 0
#define PWCLO_STREAM_LAYOUT_HIGH 1
#define PWCLO_STREAM_LAYOUT_LOW 2
#define PWCLO_STREAM_LAYOUT_MIXED 3
int pwclo_stream_set_create_ex(int n, int layout, long long *handle);
/* The probe.  Every create call measures once how many of the set's streams run side by side and the set keeps the
 * answer; these two only read it.  The measurement: one workgroup of 64 threads per stream, launched back to back, each
 * running a fixed number of rounds of a dependent integer chain -- no memory traffic, nothing it waits for, so it ends by
 * itself -- sized to about 0.5 ms by one calibration launch on stream 0, and stamping its start and end on the constant
 * 100 MHz clock into a small device buffer of the set.  After one hipStreamSynchronize per stream the host takes the
 * largest group of launches whose intervals overlap pairwise by more than half the longer one's length (of equal groups
 * the one with the lowest stream indices).  side_by_side: that group's size, 1 .. n.  layout: the PWCLO_STREAM_LAYOUT_*
 * in effect (never _AUTO); together: bit i set = stream i belongs to the group; probe_ns: the longest probe launch. */
int pwclo_stream_set_concurrency(long long handle, int *side_by_side);
int pwclo_stream_set_probe(long long handle, int *layout, unsigned *together, long long *probe_ns);
/* n of the set; -PWCLO_EINVAL for a handle that is not live. */
int pwclo_stream_set_size(long long handle);
int pwclo_stream_set_stream(long long handle, int i, void **hip_stream);
/* Work queued on stream i after this call starts after everything queued on other_stream before it (NULL = the null
 * stream; stream i itself: nothing to do). */
int pwclo_stream_set_wait_stream(long long handle, int i, void *other_stream);
/* Slot completion, slot in [0, PWCLO_STREAM_SET_MAX): _record marks the current end of stream i as the completion of
 * `slot`; _query returns 1 when that point has been reached (or the slot was never recorded), 0 when not yet, a negative
 * error code otherwise; _wait_slot makes waiting_stream (any stream) wait for it; _synchronize_slot makes the host wait. */
int pwclo_stream_set_record(long long handle, int slot, int i);
int pwclo_stream_set_query(long long handle, int slot);
int pwclo_stream_set_wait_slot(long long handle, int slot, void *waiting_stream);
int pwclo_stream_set_synchronize_slot(long long handle, int slot);
/* The host waits for all n streams. */
int pwclo_stream_set_synchronize(long long handle);
/* Waits for the DEVICE (work on the set's streams, and work elsewhere that waits for the set's events), then destroys the
 * events and streams.  The handle is refused from then on. */
int pwclo_stream_set_destroy(long long handle);

/* ---- 1. the nine reference launchers ------------------------------------------------------ */

/* sampling.cpp:4-6 / sampling_gpu.cu:22-30.  out[b,c,j] = points[b,c,idx[b,j]].
 * points (b,c,n) f32, idx (b,npoints) i32, out (b,c,npoints) f32. */
void gather_points_kernel_wrapper(int b, int c, int n, int npoints, const float *points,
                                  const int *idx, float *out);

/* sampling.cpp:7-9 / sampling_gpu.cu:49-57.  grad_points[b,c,idx[b,j]] += grad_out[b,c,j];
 * grad_points (b,c,n) must be zero-filled by the caller (sampling.cpp:51-53). */
void gather_points_grad_kernel_wrapper(int b, int c, int n, int npoints, const float *grad_out,
                                       const int *idx, float *grad_points);

/* sampling.cpp:11-13 / sampling_gpu.cu:175-229.  Iterative furthest point sampling.
 * dataset (b,n,3) f32; temp (b,n) f32 scratch pre-filled with 1e10 by the caller
 * (sampling.cpp:74-76).  This implementation keeps the running distances in registers: temp may be
 * NULL for n <= 24576; for larger clouds it must be the (b,n) buffer (8-byte aligned) and is used --
 * and overwritten -- as the exchange workspace of the cooperative multi-workgroup sampler (or, with
 * PWCLO_FPS_COOP=0, as the running distances of the streaming fallback).  idxs (b,m) i32.  Index 0 is always the
 * first sample; points with x*x+y*y+z*z <= 1e-3 are never selected; ties are resolved exactly
 * as the reference's block-of-opt_n_threads(n) tree reduction does ("FPS tie rule"). */
void furthest_point_sampling_kernel_wrapper(int b, int n, int m, const float *dataset,
                                            float *temp, int *idxs);

/* group_points.cpp:4-6 / group_points_gpu.cu:30-39.  out[b,c,j,k] = points[b,c,idx[b,j,k]].
 * points (b,c,n), idx (b,npoints,nsample) i32, out (b,c,npoints,nsample). */
void group_points_kernel_wrapper(int b, int c, int n, int npoints, int nsample,
                                 const float *points, const int *idx, float *out);

/* group_points.cpp:8-10 / group_points_gpu.cu:66-75.  Scatter-add of grad_out (b,c,npoints,
 * nsample) into zero-filled grad_points (b,c,n). */
void group_points_grad_kernel_wrapper(int b, int c, int n, int npoints, int nsample,
                                      const float *grad_out, const int *idx, float *grad_points);

/* ball_query.cpp:4-6 / ball_query_gpu.cu:46-54.  For each centre new_xyz[b,j] the first
 * `nsample` indices k (ascending) with |new_xyz-xyz[k]|^2 < radius^2; unfilled slots repeat the
 * first hit; a centre without any hit leaves its slots untouched (caller zero-fills idx,
 * ball_query.cpp:19-21).  new_xyz (b,m,3), xyz (b,n,3), idx (b,m,nsample) i32. */
void query_ball_point_kernel_wrapper(int b, int n, int m, float radius, int nsample,
                                     const float *new_xyz, const float *xyz, int *idx);

/* interpolate.cpp:4-5 / interpolate_gpu.cu:61-68.  Three nearest `known` points of every
 * `unknown` point: dist2 (b,n,3) squared distances ascending, idx (b,n,3); ties -> lower index;
 * m < 3 leaves dist2 = +inf, idx = 0 in the unfilled slots. */
void three_nn_kernel_wrapper(int b, int n, int m, const float *unknown, const float *known,
                             float *dist2, int *idx);

/* interpolate.cpp:6-8 / interpolate_gpu.cu:103-111.
 * out[b,c,j] = sum_t points[b,c,idx[b,j,t]] * weight[b,j,t].  points (b,c,m), out (b,c,n). */
void three_interpolate_kernel_wrapper(int b, int c, int m, int n, const float *points,
                                      const int *idx, const float *weight, float *out);

/* interpolate.cpp:9-12 / interpolate_gpu.cu:145-154.  Scatter-add of grad_out (b,c,n) * weight
 * into zero-filled grad_points (b,c,m). */
void three_interpolate_grad_kernel_wrapper(int b, int c, int n, int m, const float *grad_out,
                                           const int *idx, const float *weight,
                                           float *grad_points);

/* ---- 2. native replacements of pure-PyTorch ops on the same path -------------------------- */

/* Replaces pytorch_utils.py:12-49 (knn_point = dense distance + torch.topk).  For every query
 * new_xyz[b,j] the `nsample` nearest points of xyz[b] in ascending key order, key =
 * sqrtf(((dx*dx + dy*dy) + dz*dz) + 1e-8f) with dx = query - candidate, every operation rounded
 * to binary32 (no contraction); equal keys -> lower index first.  xyz (b,n,3), new_xyz (b,s,3),
 * idx (b,s,nsample) i32, dist (b,s,nsample) f32 or NULL.  Requires 1 <= nsample <= 64 and
 * nsample <= n (else PWCLO_EINVAL). */
void knn_point_kernel_wrapper(int b, int n, int s, int nsample, const float *xyz,
                              const float *new_xyz, int *idx, float *dist);

/* Same result through an exact spatially pruned search (Morton-sorted candidate blocks with
 * bounding boxes) when 256 <= n <= 16384: needs a caller-provided device workspace of
 * knn_point_workspace_bytes(b, n) bytes (0 = not applicable: the exhaustive kernel is used and
 * `workspace` may be NULL; also used when s < 256, where the build does not amortise).
 * Bit-identical output to knn_point_kernel_wrapper. */
long long knn_point_workspace_bytes(int b, int n);
/* The workspace's two cloud-major sections, rows then boxes: out[0..3] = (rows offset, rows bytes per cloud, boxes
 * offset, boxes bytes per cloud), so that rows offset + b * rows bytes = boxes offset and boxes offset + b * boxes bytes =
 * knn_point_workspace_bytes(b, n).  Returns 1; 0 with out all zero where there is no workspace (exhaustive kernel). */
int knn_point_workspace_sections(int b, int n, long long *out);
/* The two passes of the pruned search separately, so that ONE build of a cloud's search structure serves several
 * searches and the slab-pruned sampler below: workspace of knn_point_build_bytes(b, n) bytes (64 <= n <= 16384);
 * slab_tab (optional, b*32 ints): (padded first row, row count) of the cloud's knn_point_slabs(n) <= 16 x-slabs. */
long long knn_point_build_bytes(int b, int n);
int knn_point_slabs(int n);
void knn_build_kernel_wrapper(int b, int n, const float *xyz, void *workspace, int *slab_tab);
void knn_point_prebuilt_kernel_wrapper(int b, int n, int s, int nsample, const float *new_xyz, int *idx, float *dist,
                                       void *workspace);
/* The same search on clouds [first_cloud, first_cloud + b) of a structure that knn_build / knn_point_ws built for
 * built_b >= first_cloud + b clouds of n points (the pyramid builds both frames' clouds as one batch; a refinement level
 * searches one frame's half of it without rebuilding).  new_xyz (b,s,3), idx (b,s,nsample). */
void knn_point_prebuilt_slice_kernel_wrapper(int b, int n, int s, int nsample, const float *new_xyz, int *idx,
                                             float *dist, void *workspace, int first_cloud, int built_b);
/* The spatial order the sorted sampler below wants, built on the device: points (b,n,3) -> sorted (b,n,3), perm (b,n);
 * workspace of fps_spatial_order_workspace_bytes(b, n) bytes.  (32^3 Morton cells by counting sort, then every block of
 * 1024 consecutive positions sorted by sampling priority; any such order is exact for the sampler.) */
long long fps_spatial_order_workspace_bytes(int b, int n);
void fps_spatial_order_kernel_wrapper(int b, int n, const float *points, float *sorted, int *perm, void *workspace);
/* Large clouds (n > 24576) presented in a spatially coherent order: sorted (b,n,3) = dataset gathered by perm (b,n),
 * perm[p] = original index of sorted position p; inside every block of 1024 consecutive positions the positions are
 * ordered by ascending sampling priority (bitrev(k mod bs) << 23 | k div bs of the original index k).  A wave of the
 * cooperative sampler then owns a compact cell and skips its distance update -- exactly -- whenever the new sample is
 * farther from the cell's box than the largest running distance.  Same idxs (ORIGINAL numbering) / new_xyz as
 * furthest_point_sampling_xyz_kernel_wrapper, bit for bit.  temp: the (b,n) scratch, 8-byte aligned. */
void furthest_point_sampling_sorted_kernel_wrapper(int b, int n, int m, const float *dataset, const float *sorted,
                                                   const int *perm, float *temp, int *idxs, float *new_xyz);
/* furthest_point_sampling_chain_kernel_wrapper for a cloud whose search structure exists (knn_point_slabs(n) == 8,
 * n >= 4096: level 1 of the pyramid): the distance update of a wave is skipped, exactly, whenever the new sample
 * cannot lower any running distance inside the wave's x-slab (csrc/sampling.hip: fps_slab_kernel).  status: b ints
 * (device) the two kernels use to divide the clouds between them.  Same idxs / new_xyz / tie_out as the chain entry. */
void furthest_point_sampling_slab_kernel_wrapper(int b, int n, int m, const float *dataset, int *idxs,
                                                 float *new_xyz, int *tie_out, int tie_iters,
                                                 const void *knn_workspace, const int *slab_tab, int *status);
void knn_point_ws_kernel_wrapper(int b, int n, int s, int nsample, const float *xyz,
                                 const float *new_xyz, int *idx, float *dist, void *workspace);

/* Replaces PWCLO_utils.py:42-63 (warp): out = q (x) (0,xyz) (x) q^-1 + t, scalar-first
 * quaternions, q^-1 = conj(q) / (|q|^2 + 1e-10).  xyz, out (b,3,n); q (b,4); t (b,3). */
void quat_warp_kernel_wrapper(int b, int n, const float *xyz, const float *q, const float *t,
                              float *out);

/* ---- 3. fused eval-mode layers ------------------------------------------------------------- */
/* One launch per reference module forward (eval mode: BatchNorm running statistics folded into
 * the packed weights, no dropout).  Feature tensors are POINT-MAJOR (b, n, c) fp32 with c a
 * multiple of 16; `packed_w` is produced by pwclonet_pylidarslam_amd/fused.py (layout in
 * csrc/mlp_core.hpp).  Unsupported channel configurations record PWCLO_EINVAL. */

/* PointnetSAModulePWCLONet.forward after FPS/knn (pointnet2_modules.py:205-243): gather the k
 * neighbours idx[b,s,:] of every query, subtract the query centre, run the 3-layer shared MLP
 * (padded widths c1,c2,c3) and max over the neighbours.  xyz (b,n,3), new_xyz (b,s,3), feat
 * (b,n,c_feat) or NULL when c_feat == 0 (level-0 input [xyz_diff, grouped_xyz]), idx (b,s,k)
 * i32, out (b,s,c3). */
void sa_fused_kernel_wrapper(int b, int n, int s, int k, int c_feat, int c1, int c2, int c3,
                             const float *xyz, const float *new_xyz, const float *feat,
                             const int *idx, const float *packed_w, float *out);

/* furthest_point_sampling_kernel_wrapper that also writes the sampled coordinates new_xyz (b,m,3)
 * = dataset[b, idxs[b,j], :] (the gather_operation that always follows FPS in the set-abstraction
 * layer, pointnet2_modules.py:196-203); new_xyz may be NULL. */
void furthest_point_sampling_xyz_kernel_wrapper(int b, int n, int m, const float *dataset,
                                                float *temp, int *idxs, float *new_xyz);

/* The same for a CHAIN of samplers (the pyramid: each level samples the previous level's samples).
 * Sampling a cloud that is itself an FPS sample list, in sampling order, returns its prefix 0..m-1
 * whenever every arg-max of the producing call was unique; an exact two-point distance tie that the
 * producer resolved over two consecutive iterations shows up as an adjacent pair in an order decided by
 * the child's position priorities (csrc/sampling.hip, "Sampling chains").
 *   tie_out  (b, 12) i32 or NULL: per cloud [fallback flag, number of tie events, 8 event iterations, -, -]
 *            for the first tie_iters - 1 decisions of THIS call (needs m >= tie_iters + 2, else flag = 1);
 *   prefix_in (b, 12) i32 or NULL: records written by the call that produced `dataset`; clouds whose
 *            flag is 0 get their result written directly (m must be <= that call's tie_iters), all
 *            others run the full algorithm.  Outputs are identical either way. */
void furthest_point_sampling_chain_kernel_wrapper(int b, int n, int m, const float *dataset, float *temp,
                                                  int *idxs, float *new_xyz, int *tie_out, int tie_iters,
                                                  const int *prefix_in);

/* Input adapter (pwclo_net.py:125-126 and the siamese batching): xyz_f1, xyz_f2 (b,3,n) channel-major
 * -> out (2b,n,3) point-major, frame 1 first. */
void ingest_pairs_kernel_wrapper(int b, int n, const float *xyz_f1, const float *xyz_f2, float *out);

/* The same batch straight from the prediction module's inputs (slam/training/prediction_modules.py:
 * 144-160: `pcd[:, :num_points, :3]` then permute): frame1/frame2 (b, n_total, c) point-major with
 * c >= 3 floats per point; the first n points and first 3 channels of each -> out (2b, n, 3). */
void ingest_frames_kernel_wrapper(int b, int n, int n_total, int c, const float *frame1,
                                  const float *frame2, float *out);

/* Sequence form of ingest_frames (FusedPWCLONet.sample_sequence): frames (t, n_total, c) point-major, c >= 3;
 * the first n points and first 3 channels of each frame -> out (t, n, 3), frame order kept. */
void ingest_sequence_kernel_wrapper(int t, int n, int n_total, int c, const float *frames, float *out);

/* Hamilton product of quaternion rows (PW/PWCLO_utils.py:83-95 mul_q_point, :117-129 mul_point_q -- the same
 * component expressions): out (b,4,n) = a (b,4,na) (x) q (b,4,nb), na and nb each 1 (broadcast) or n; conj_a / conj_b
 * != 0 use that operand's conjugate.  Products rounded before the left-to-right sums: the torch expression bit for
 * bit.  The product's gradients are products with conjugates, so the training path's backward calls this again. */
void hamilton_product_kernel_wrapper(int b, int n, int na, int nb, int conj_a, int conj_b, const float *a,
                                     const float *q, float *out);

/* quat_warp_kernel_wrapper on point-major clouds: xyz, out (b,n,3). */
void quat_warp_pm_kernel_wrapper(int b, int n, const float *xyz, const float *q, const float *t,
                                 float *out);

/* PointnetFPModulePWCLONet.forward, knn branch up to the max over neighbours
 * (pointnet2_modules.py:479-506): gather feat1 (b,n,64) and xyz1 (b,n,3) at idx (b,s,k<=8), append
 * xyz1[nbr]-xyz2[s], shared MLP 67->128->64, max over k.  out (b,s,64). */
void upconv_fused_kernel_wrapper(int b, int n, int s, int k, const float *xyz2, const float *xyz1,
                                 const float *feat1, const int *idx, const float *packed_w,
                                 float *out);

/* Shared MLP (1 or 2 layers, padded widths w1,w2; w2 = 0 for one layer) over the channel
 * concatenation of up to three per-point tensors src_i (b,s,c_i): the set-upconv post_mlp
 * (pointnet2_modules.py:508-515) and FlowPredictor.forward (PW/flowpredictor.py:53-83). */
void pointwise_fused_kernel_wrapper(int b, int s, int c0, int c1, int c2, int w1, int w2,
                                    const float *src0, const float *src1, const float *src2,
                                    const float *packed_w, float *out);

/* The same two-layer stack followed by ONE linear layer (w2 -> wt channels, bias, no activation) applied to the stack's
 * output while it is in registers and written to out_tail (b,s,wt): the hoisted partial product W1_feat . out + b1 that the
 * next refinement level's set-upconv (pointnet2_modules.py:479-506, first layer of its mlp) would otherwise request from
 * linear_jobs_kernel_wrapper (section 4); same rows bit for bit.  packed_tail holds tail_floats floats. */
void pointwise_tail_fused_kernel_wrapper(int b, int s, int c0, int c1, int c2, int w1, int w2, int wt,
                                         const float *src0, const float *src1, const float *src2,
                                         const float *packed_w, const float *packed_tail, float *out,
                                         float *out_tail, int tail_floats);

/* CostVolume.forward (PW/costvolume.py:63-190) in three launches.
 * a1: per (query s, neighbour k) pixel: mlp_convs([geometry10 | feat1[s] | feat2[idx]]) -> pix
 *     (b, s*pix_slots, 64).  pix_slots is the CALLER's choice (it allocates pix) and must be passed identically
 *     to a1 and a2: k rounded up to 8/16/32, or 6 for k == 6 (dense layout of the refinement levels).
 *     xyz1 (b,s,3), feat1 (b,s,c), xyz2 (b,n,3), feat2 (b,n,c), idx (b,s,k).
 * Packed-weight format (entry points that take `wfmt, packed_floats`): 0 = fp32 operand tiles
 *     (v_mfma_f32_16x16x4_f32), 1 = the opt-in three-term bf16 split tiles, 2 = bf16 tiles (dtype "bf16":
 *     v_mfma_f32_16x16x32_bf16 on operands rounded once, fp32 accumulate; with it the hoisted rows pre / u / v / u2 / v2
 *     and the per-pixel buffer pix are bf16 IN MEMORY too: 2 bytes per channel; csrc/mlp_core.hpp); the format is a
 *     property of the buffer, fixed when it was packed.  packed_floats = its length; a length that does not match
 *     the layout the selected kernel indexes is refused with PWCLO_EINVAL (never read out of bounds).
 * a2: mlp_conv_xyz_1(geometry10), mlp2_convs, softmax over k, sum_k w*pix -> out (b,s,64).
 * b : second aggregate over the k<=4 frame-1 neighbours idx (b,s,k) of each frame-1 point:
 *     mlp_conv_xyz_2, mlp3_convs([enc | feat1[s] | first[idx]]), softmax, sum_k w*first[idx]. */
void cv_fused_a1_kernel_wrapper(int b, int n, int s, int k, int c, const float *xyz1,
                                const float *feat1, const float *xyz2, const float *feat2,
                                const int *idx, const float *packed_w, float *pix, int pix_slots);
void cv_fused_a2_kernel_wrapper(int b, int n, int s, int k, const float *xyz1, const float *xyz2,
                                const int *idx, const float *packed_w, const float *pix, float *out,
                                int pix_slots, int wfmt, int packed_floats);
void cv_fused_b_kernel_wrapper(int b, int s, int k, int c, const float *xyz1, const float *feat1,
                               const float *first, const int *idx, const float *packed_w, float *out);

/* out[b,c] = sum_n emb[b,n,c] * softmax_n(mask[b,n,c]) for 64-channel point-major emb/mask
 * (b,n,64): F.softmax(mask, dim=2) + the masked sum of PoseCalculator.forward
 * (PW/pose_calculator.py:58). */
void masked_pool_kernel_wrapper(int b, int n, const float *emb, const float *mask, float *out);

/* Whole pose head of one pyramid level in one launch: the masked pooling above, PoseCalculator's
 * three 1x1 convolutions (w_qt (256,64), w_q (4,256), w_t (3,256) + biases; eval mode, dropout =
 * identity; PW/pose_calculator.py:47-86), and -- when q_prev (b,4) / t_prev (b,3) are given --
 * the pose composition of PoseWarpRefinement (PW/pose_warp_refinement.py:139,148).  Writes q_out
 * (b,4), t_out (b,3) and this level's row [t, q/|q|] at pose_row + i*row_stride (pwclo_net.py:195-205). */
void pose_head_fused_kernel_wrapper(int b, int n, const float *emb, const float *mask,
                                    const float *w_qt, const float *b_qt, const float *w_q,
                                    const float *b_q, const float *w_t, const float *b_t,
                                    const float *q_prev, const float *t_prev, float *q_out,
                                    float *t_out, float *pose_row, int row_stride);

/* The same, followed in the same launch by the next (finer) level's quat_warp_pm(warp_src (b,warp_n,3), q_out, t_out) ->
 * warp_out: bit-identical to the two separate launches (PW/pose_warp_refinement.py:104-106 is the first thing the next
 * level does with this pose). */
void pose_head_warp_fused_kernel_wrapper(int b, int n, const float *emb, const float *mask,
                                         const float *w_qt, const float *b_qt, const float *w_q,
                                         const float *b_q, const float *w_t, const float *b_t,
                                         const float *q_prev, const float *t_prev, float *q_out,
                                         float *t_out, float *pose_row, int row_stride, int warp_n,
                                         const float *warp_src, float *warp_out);

/* Deterministic (atomics-free) form of group_points_grad / gather_points_grad (nsample = 1): the caller
 * supplies the inverse of idx per cloud -- perm (b, npoints*nsample) i32 = positions p sorted by idx[b,p]
 * (stable: ascending p inside a source point), seg (b, n+1) i32 = segment starts -- and every
 * grad_points[b,c,i] is the sum of grad_out[b,c,perm[seg[i]..seg[i+1])] in that order.  No zero fill. */
void group_points_grad_sorted_kernel_wrapper(int b, int c, int n, int npoints, int nsample,
                                             const float *grad_out, const int *perm, const int *seg,
                                             float *grad_points);

/* Channel-slice forms of the three grouping entry points.  The reference concatenates every grouped tensor with the
 * coordinate differences / the other frame's features before the shared MLP (P2/pointnet2_modules.py:222-230, 490-500;
 * PW/costvolume.py:107, 134, 172), i.e. it writes the grouped tensor, then copies it into the concatenated one, and in
 * backward copies the slice of the gradient back out.  Here `out` / `grad_out` point at channel `c_off` of cloud 0 of a
 * (b, c_total, npoints, nsample) tensor and `batch_stride` = c_total * npoints * nsample floats: the kernels group
 * straight into / differentiate straight out of the concatenated tensor.  Values are those of the dense entry points. */
void group_points_strided_kernel_wrapper(int b, int c, int n, int npoints, int nsample, const float *points,
                                         const int *idx, float *out, long long batch_stride);
void group_points_grad_strided_kernel_wrapper(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                                              long long batch_stride, const int *idx, float *grad_points);
void group_points_grad_sorted_strided_kernel_wrapper(int b, int c, int n, int npoints, int nsample,
                                                     const float *grad_out, long long batch_stride, const int *perm,
                                                     const int *seg, float *grad_points);

/* Inputs of the cost volume's shared MLPs (PW/costvolume.py:92-107 first aggregate, :155-172 second): the 10-channel
 * geometry encoding of every (centre p, neighbour q = src[idx]) pair, out[b, 0:10, j, t] = [p (3), q (3), q - p (3),
 * sqrt(sum (q - p)^2 + 1e-20)], and the centre's features tiled over the k neighbours (torch.tile in the reference),
 * written straight into their channel slice of the concatenated tensor (`out` = first channel of the slice in cloud 0,
 * batch_stride floats between clouds, as the *_strided grouping entry points).  centre_xyz (b,3,s), src_xyz (b,3,n),
 * idx (b,s,k) i32, feats (b,c,s).  Forward values are the reference's bit for bit.  Gradients: d_centre_xyz (b,3,s) is
 * written; d_src_xyz (b,3,n) must be zero-filled and receives atomic adds; either may be NULL (not wanted); d_pair
 * (b,3,s,k), instead of d_src_xyz, receives the neighbours' gradients pair by pair (for group_points_grad_sorted).
 * broadcast_centre_grad: d_feats (b,c,s) = sum over the k neighbours of the slice's gradient. */
void geometry_encode_kernel_wrapper(int b, int n, int s, int k, const float *centre_xyz, const float *src_xyz,
                                    const int *idx, float *out, long long batch_stride);
void geometry_encode_grad_kernel_wrapper(int b, int n, int s, int k, const float *centre_xyz, const float *src_xyz,
                                         const int *idx, const float *grad_out, long long batch_stride,
                                         float *d_centre_xyz, float *d_src_xyz, float *d_pair);
/* out[b, 0:3, j, t] = src_xyz[b, :, idx[b,j,t]] - centre_xyz[b, :, j] (P2/pointnet2_modules.py:215-218, 485-488), into a
 * channel slice like the entries above; its gradient is group_points_grad_strided (neighbours) and minus
 * broadcast_centre_grad (centres) of the same slice. */
void xyz_diff_kernel_wrapper(int b, int n, int s, int k, const float *centre_xyz, const float *src_xyz, const int *idx,
                             float *out, long long batch_stride);
void broadcast_centre_kernel_wrapper(int b, int c, int s, int k, const float *feats, float *out, long long batch_stride);
void broadcast_centre_grad_kernel_wrapper(int b, int c, int s, int k, const float *grad_out, long long batch_stride,
                                          float *d_feats);

/* On-device front end of the dataset (slam/dataset/kitti_odometry_dataset.py:375-397, filter_pcd
 * :149-160): points (n,4) f32 raw velodyne rows (x,y,z,intensity), tr (12) f64 DEVICE array = rows of the
 * 3x4 calibration matrix Tr; xyz (n,3) f32 = Tr . (x,y,z,1) evaluated in fp64, keep (n) i32 = 1 where the
 * transformed point is not ground (y <= 1.1) and within |x| < 30, |z| < 30. */
void kitti_transform_filter_kernel_wrapper(int n, const double *tr, const float *points, float *xyz, int *keep);

/* KITTI-360 variant (slam/dataset/kitti_360_dataset_2.py:113-123; no calibration transform): xyz (n,3) = the
 * first three columns, keep = not ground (z >= ground_z, the reference's -(1.73 - 0.3)) and |x| < near and
 * |y| < near, compared in fp32.  n may span several frames laid end to end (b*n rows). */
void kitti360_filter_kernel_wrapper(int n, float ground_z, float near, const float *points, float *xyz, int *keep);

/* Stable per-frame compaction after either filter: keep (b,n) i32, any non-zero word keeps the row; the kept rows of
 * frame f are copied in frame order to out[f, 0 .. count-1] (out (b,cap,3) f32, zero-filled by the caller: zero rows are
 * never selected by furthest_point_sampling; kept rows beyond cap are dropped), counts (b) i32 = min(kept, cap).  The
 * scan is inside the kernel: one workgroup per frame, ballot / popcount slots. */
void compact_frames_scan_kernel_wrapper(int b, int n, int cap, const int *keep, const float *xyz, float *out, int *counts);
/* Filter + compaction of S raw sweeps of different lengths in one launch (one workgroup per stream): sweeps (S,R,4) f32
 * with row stride R (16-byte aligned), lengths (S) i32 in DEVICE memory (clamped to [0, R]; only rows [0, lengths[s])
 * are read).  dataset 0: KITTI, tr (S,3,4) f64 per-stream calibration on the device (ground_z / near unused); dataset 1:
 * KITTI-360 with ground_z / near (tr unused).  Same per-row arithmetic as the two filters above.  packed (S,cap,3) f32:
 * survivors in frame order, then zero rows up to cap, ALL written by the kernel (no caller zero-fill); counts (S) i32 =
 * min(kept, cap). */
void sweep_filter_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps, int dataset,
                                         const double *tr, float ground_z, float near, float *packed, int *counts);

/* Voxel grid sampling (preprocess.grid_sample): one row per occupied voxel, the lowest-index one.
 * q_a = rint((double)p_a / voxel) (fp64 division, half to even), h = 73856093 q_x + 19349669 q_y + 83492791 q_z in 64 bits
 * with wraparound; a row is a winner iff no lower-index candidate row of its cloud has its h.  Rows with a non-finite
 * coordinate or |p_a / voxel| >= 2^31 are no candidates.  One workgroup per cloud and an open-addressing table in the
 * caller's workspace, cleared by the launch itself (nothing persists between launches; graph-capturable).
 * Bytes of workspace for b clouds of up to n rows (8-byte aligned; 0 when b or n is out of range, n <= 2^20). */
long long grid_sample_workspace_bytes(int b, int n);
/* points (b,n,stride) f32 with stride 3 or 4 floats per row; lengths (b) i32 in DEVICE memory or null (all n rows; clamped
 * to [0, n]); keep_in (b,n) i32 or null: rows with 0 are no candidates.  keep_out (b,n) i32 = 1 for the winners, 0
 * elsewhere (all n entries written); counts (b) i32 = winners per cloud. */
void grid_sample_keep_kernel_wrapper(int b, int n, int stride, const float *points, const int *lengths, const int *keep_in,
                                     double voxel, void *workspace, int *keep_out, int *counts);
/* sweep_filter_compact_kernel_wrapper with the grid between the filter and the compaction: the candidates are the rows the
 * filter keeps, keyed on the coordinates it outputs.  workspace: grid_sample_workspace_bytes(S, R).  packed (S,cap,3): the
 * winners in row order, then zero rows; winners (S) i32 = the number of winners, counts (S) i32 = min(winners, cap). */
void sweep_filter_grid_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps, int dataset,
                                              const double *tr, float ground_z, float near, double voxel, void *workspace,
                                              float *packed, int *counts, int *winners);

/* Motion compensation of raw sweeps (preprocess.deskew; the reference's `distortion` filter fed by its
 * constant-velocity initialisation).  For one cloud with fp32 coordinates p_i as the filter outputs them, a time tau_i per
 * row and a motion given as a pose row [tx ty tz qw qx qy qz] (fp32):
 *   1. candidates are the rows the filter keeps; the keep decision is taken on the coordinates BEFORE de-skewing, so masks
 *      and survivor counts are those without the step;
 *   2. tau_min / tau_max = minimum / maximum over the candidates below the cloud's length whose time is finite;
 *      alpha_i = (tau_i - tau_min) / (tau_max - tau_min) in fp64; alpha_i = 0 for every row if tau_max == tau_min or no
 *      candidate has a finite time, and for a candidate whose own time is not finite; other rows have no influence;
 *   3. q = (w, x, y, z) in fp64, nq = |q|^2; nq < 1e-8: the identity rotation; else q^ = q / sqrt(nq), negated if w < 0
 *      (the shortest arc), theta = 2 atan2(|v|, w), axis k = v / |v| (any unit vector if |v| = 0); R(alpha) = the rotation
 *      by alpha * theta about k (= SciPy's Slerp([0, 1], [I, R])(alpha) for R = quat2mat(q));
 *   4. p'_i = R(alpha_i) p_i + alpha_i t, in fp64 from the fp32 inputs, rounded to fp32 once;
 *   5. a row with alpha_i = 0, and every row of a cloud whose motion is the identity (theta = 0, t = 0), keeps p_i's bits;
 *   6. in the front end: filter -> de-skew -> voxel grid (if any) -> compaction -> sampler.
 * The op alone: points (b,n,stride) f32 with stride 3 or 4, times (b,n) f64, motion (b,7) f32, lengths (b) i32 in DEVICE
 * memory or null (all n rows; clamped to [0, n]), keep_in (b,n) i32 or null (all rows).  xyz (b,n,3) f32, all n rows
 * written; non-candidates pass through unchanged.  One workgroup per cloud; graph-capturable. */
void deskew_rows_kernel_wrapper(int b, int n, int stride, const float *points, const double *times, const float *motion,
                                const int *lengths, const int *keep_in, float *xyz);
/* sweep_filter_compact_kernel_wrapper with the de-skew between the filter and the compaction: times (S,R) f64 with row
 * stride R, motion (S,7) f32 in DEVICE memory (read by the launch: a captured graph follows it).  restart, have_prev (S)
 * i32 or null (per-stream mode): stream s gets the identity motion when restart[s] != 0 or have_prev[s] == 0.  Same buffer
 * contract: all of packed[s, :cap] is written, survivors then zeros; counts as there. */
void sweep_filter_deskew_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps, int dataset,
                                                const double *tr, float ground_z, float near, const double *times,
                                                const float *motion, const int *restart, const int *have_prev,
                                                float *packed, int *counts);
/* sweep_filter_grid_compact_kernel_wrapper on the de-skewed coordinates (the grid sees what the network sees). */
void sweep_filter_deskew_grid_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps,
                                                     int dataset, const double *tr, float ground_z, float near,
                                                     const double *times, const float *motion, const int *restart,
                                                     const int *have_prev, double voxel, void *workspace, float *packed,
                                                     int *counts, int *winners);
/* After the append of a streaming step: motion[s] (S,7) f32 = the row at rows + s * row_stride floats (the level-1 pose row
 * of the pair just registered), or the identity (0,0,0, 1,0,0,0) when rows is null (after a prime).  active (S) i32 or
 * null (all): streams with active[s] == 0 keep their motion.  One workgroup, one thread per stream (S <= 1024). */
void stream_motion_handover_kernel_wrapper(int S, const int *active, const float *rows, int row_stride, float *motion);

/* Training batches from raw LiDAR pairs (batches.TrainBatchBuilder), two launches per batch.
 * state (3) i64 in DEVICE memory = {seed, next step, step of the batch in flight}; random words are Philox4x32-10 with
 * key = seed and counter = (index, cloud or pair, step mod 2^32, purpose: 0 selection keys, 1 draws with replacement,
 * 2 augmentation).
 * Pose side, one thread per pair: state[2] = state[1], state[1] += 1; mode 0: no augmentation (T_trans = I, T_gt = T_diff,
 * aug_params zeroed), 1: aug_params (B,6) f32 drawn (six clipped normals, the reference's scales and clips), 2: aug_params
 * read as the caller left them.  t_diff (B,3,4) f64; t_trans (B,3,4) f64 = [Rx.Ry.Rz(params[:3] * pi / 4) | params[3:]];
 * t_gt (B,4,4) f64 = T_diff . inv(T_trans) (dataset 0, KITTI) or T_trans . T_diff (dataset 1, KITTI-360); gt (B,7) f32 =
 * [t_gt translation, quaternion w x y z] (KITTI: through the zyx Euler angles; KITTI-360: the largest-diagonal form). */
void train_batch_pose_kernel_wrapper(int B, int dataset, int mode, long long *state, const double *t_diff, float *aug_params,
                                     double *t_trans, double *t_gt, float *gt);
/* Sample side, one 1024-thread workgroup per cloud c = 2 * pair + frame: sweeps (B,2,R,4) f32 (16-byte aligned), lengths
 * (B,2) i32 in DEVICE memory (both frames of a pair use rows [0, min of the two), clamped to [0, R]); tr (B,3,4) f64 per
 * pair (dataset 0) or ground_z / near (dataset 1): the row arithmetic of the filters above.  count >= npoints: the npoints
 * survivors with the smallest keys (word << 32 | row), in key order; 0 < count < npoints: all survivors in frame order,
 * then draws (word * count) >> 32 into that list; count == 0: draws (word * n) >> 32 over all rows.  augmented != 0: frame 1
 * of every pair is moved by t_trans (fp64, rounded once).  xyz_f1 / xyz_f2 (B,3,npoints) f32: KITTI gets (augmented frame 1,
 * frame 0), KITTI-360 (frame 0, augmented frame 1).  indices (2B,npoints) i32 = the raw row of every output point,
 * counts (2B) i32 = survivors.  npoints <= 8192; reads state[0] and state[2] as the pose launch left them. */
void train_batch_sample_kernel_wrapper(int B, int R, int npoints, int dataset, const int *lengths, const float *sweeps,
                                       const double *tr, float ground_z, float near, const long long *state,
                                       const double *t_trans, int augmented, float *xyz_f1, float *xyz_f2, int *indices,
                                       int *counts);

/* Flat gradient bucket and Adam over a list of n fp32 tensors (flat_step.FlatAdam).  The list is
 * read from HOST arrays at launch time -- tensors[t] (device pointer, 4-byte aligned), counts[t] values, offsets[t] = first
 * value in the bucket, a multiple of 64 (256 bytes) with offsets[t] + round_up(counts[t], 64) <= total - 1 -- and travels to
 * the kernels by value, flat_step_entries_per_launch() tensors per launch, so a captured graph holds it without host
 * memory.  Spans of different tensors must not overlap (flat_step.bucket_layout lays them back to back).  bucket: total
 * fp32 values, 16-byte aligned; its LAST value is the count of non-finite inputs. */
int flat_step_entries_per_launch(void);
/* bucket[offsets[t] + i] = tensors[t][i] * scale (scale 1.0f: the bits as they are); the padding up to round_up(count, 64)
 * is written as zero; bucket[total - 1] = number of NaN / +-Inf values read, as fp32 (exact below 2^24). */
void flat_pack_kernel_wrapper(int n, void *const *tensors, const long long *counts, const long long *offsets, float scale,
                              float *bucket, long long total);
/* torch.optim.Adam (decoupled == 0: weight_decay is L2, added to the gradient) or AdamW (decoupled != 0) without amsgrad /
 * maximize over tensors[t] = the PARAMETERS; gradient = bucket, exp_avg, exp_avg_sq: total fp32 values each at the same
 * offsets.  step (1) i64 and lr (1) f64 live in DEVICE memory; coef (4) f64 is scratch of the launch group.  A one-thread
 * launch goes first: bucket[total - 1] == 0 -> step += 1 and coef = {1, lr / (1 - beta1^step), sqrt(1 - beta2^step), lr};
 * otherwise coef[0] = 0 and the update launches leave parameters, moments and step as they were.  Every value is computed
 * in fp64 from the fp32 inputs and rounded once. */
void flat_adam_kernel_wrapper(int n, void *const *tensors, const long long *counts, const long long *offsets,
                              const float *bucket, float *exp_avg, float *exp_avg_sq, long long total, long long *step,
                              const double *lr, double *coef, double beta1, double beta2, double eps, double weight_decay,
                              int decoupled);
/* The same, and skipped (1) i64 in DEVICE memory counts the steps not applied: the one-thread launch adds 1 to it whenever
 * it finds bucket[total - 1] != 0.  Nothing resets it (flat_pack zeroes the bucket's count, not this). */
void flat_adam_skipped_kernel_wrapper(int n, void *const *tensors, const long long *counts, const long long *offsets,
                                      const float *bucket, float *exp_avg, float *exp_avg_sq, long long total,
                                      long long *step, const double *lr, double *coef, double beta1, double beta2,
                                      double eps, double weight_decay, int decoupled, long long *skipped);

/* ---- 3b. module-path layers: training-mode BatchNorm, stack tails, pointwise convolution ---- */

/* Training-mode BatchNorm over x (b, c, l) f32 (l = product of the trailing dimensions), the statistics pass of
 * the module path's Conv -> BN -> ReLU stacks (P2/pytorch_utils.py:86-111 wraps torch.nn.BatchNorm{1,2}d; semantics
 * of torch.nn.functional.batch_norm(training=True)): y = (x - mean) * invstd * gamma + beta with the batch's
 * mean / biased variance per channel, running_* updated in place with `momentum` and the unbiased variance
 * (both may be NULL), save_mean / save_invstd (c) kept for the backward.  gamma / beta may be NULL (1 / 0).
 * workspace: batchnorm_train_workspace_bytes(c) bytes of device memory, 8-byte aligned.  y == NULL: statistics only
 * (running_*, save_*), no apply pass -- for conv1x1_bnrelu_forward below. */
long long batchnorm_train_workspace_bytes(int c);
/* relu != 0 fuses the stack's following ReLU: y = max(., 0), and the backward masks dy where that output was 0
 * (the mask is recomputed from x, nothing extra is saved). */
void batchnorm_train_forward_kernel_wrapper(int b, int c, int l, const float *x, const float *gamma,
                                            const float *beta, float eps, float momentum, float *running_mean,
                                            float *running_var, float *y, float *save_mean, float *save_invstd,
                                            void *workspace, int relu);
/* The *_devmom siblings of the three entry points that take `float momentum` read it from DEVICE memory instead:
 * momentum_dev (1) f32, loaded by the one lane per channel that writes running_*, same arithmetic ((1 - (double)m) *
 * running + (double)m * value, rounded once), so a cell holding m gives the bits the argument m gives.  A launch argument
 * is baked into a captured graph's kernel node; the cell is re-read by every replay, so a momentum schedule needs no
 * recapture.  momentum_dev == NULL with running_mean != NULL is a caller error (PWCLO_EINVAL). */
void batchnorm_train_forward_devmom_kernel_wrapper(int b, int c, int l, const float *x, const float *gamma,
                                                   const float *beta, float eps, const float *momentum_dev,
                                                   float *running_mean, float *running_var, float *y, float *save_mean,
                                                   float *save_invstd, void *workspace, int relu);
/* dx (b, c, l), dgamma (c), dbeta (c) from dy (the gradient w.r.t. the forward's output) and the saved statistics. */
void batchnorm_train_backward_kernel_wrapper(int b, int c, int l, const float *x, const float *dy,
                                             const float *gamma, const float *beta, const float *save_mean,
                                             const float *save_invstd, float *dx, float *dgamma, float *dbeta,
                                             void *workspace, int relu);

/* Tail of the module path's grouped stacks in training mode: BatchNorm (batch statistics) -> ReLU -> max over the k
 * neighbours (P2/pointnet2_modules.py: `self.mlp_module(new_features)` followed by `.max(dim=3)` /
 * F.max_pool2d(kernel=[1, nsample]); the reference materialises the (b, c, s, k) activation between them).
 * x (b, c, s, k) f32 = the last convolution's output, k in {4, 8, 16, 32}; pooled (b, c, s) f32; arg (b, c, s) u8 =
 * first neighbour reaching the maximum; xsel (b, c, s) f32 = x at arg.  Statistics, running_* update, save_* and
 * workspace as batchnorm_train_forward_kernel_wrapper.  Same values as BN -> ReLU -> max evaluated separately. */
void batchnorm_train_relu_maxk_forward_kernel_wrapper(int b, int c, int s, int k, const float *x, const float *gamma,
                                                      const float *beta, float eps, float momentum,
                                                      float *running_mean, float *running_var, float *pooled,
                                                      unsigned char *arg, float *xsel, float *save_mean,
                                                      float *save_invstd, void *workspace);
void batchnorm_train_relu_maxk_forward_devmom_kernel_wrapper(int b, int c, int s, int k, const float *x,
                                                             const float *gamma, const float *beta, float eps,
                                                             const float *momentum_dev, float *running_mean,
                                                             float *running_var, float *pooled, unsigned char *arg,
                                                             float *xsel, float *save_mean, float *save_invstd,
                                                             void *workspace);
/* dx (b, c, s, k), dgamma (c), dbeta (c) from dpool (b, c, s), the gradient w.r.t. pooled: the dense gradient of the
 * activation (dpool at arg where the pooled value was positive, 0 elsewhere) is never written. */
void batchnorm_train_relu_maxk_backward_kernel_wrapper(int b, int c, int s, int k, const float *x, const float *dpool,
                                                       const unsigned char *arg, const float *xsel,
                                                       const float *gamma, const float *beta, const float *save_mean,
                                                       const float *save_invstd, float *dx, float *dgamma,
                                                       float *dbeta, void *workspace);

/* Pointwise convolution of the module path's shared MLPs, forward and both gradients, on channel-major rows
 * (P2/pytorch_utils.py:114-167: Conv2d(kernel_size=(1,1), bias=False) inside SharedMLP, pytorch_utils.py:12-37;
 * the reference runs torch.nn.Conv2d = cuDNN there).  x (b, cin, p), y (b, cout, p), p = product of the trailing
 * dimensions, p % 4 == 0, all pointers 16-byte aligned, cin and cout <= 512 with the packed weights within 150 KiB
 * of LDS (ceil(cin/16) * min(ceil(cout/16), 8) KiB).  fp32 FMAs on the matrix cores: equal to any fp32 convolution
 * up to summation order.
 *   transposed = 0: y[b][o][q] = sum_i w[o * cin + i] x[b][i][q]            (w (cout, cin) row-major: forward)
 *   transposed = 1: y[b][o][q] = sum_i w[i * cout + o] x[b][i][q]           (w (cin, cout) row-major: the input
 *                   gradient of the layer whose weight is w, called with x = dY, cin = the layer's cout). */
void conv1x1_forward_kernel_wrapper(int b, int cin, int cout, int p, const float *x, const float *w, int transposed,
                                    float *y);
/* The forward with the layer's eval-mode BatchNorm and ReLU in the epilogue (P2/pytorch_utils.py:114-167: conv -> bn ->
 * ReLU blocks in eval mode): y = act(conv(x) * scale[o] + shift[o]), scale = gamma / sqrt(running_var + eps), shift =
 * beta - running_mean * scale (both (cout) f32, computed by the caller), act = ReLU when relu != 0. */
void conv1x1_affine_forward_kernel_wrapper(int b, int cin, int cout, int p, const float *x, const float *w,
                                           const float *scale, const float *shift, int relu, float *y);
/* Training mode, interior layers of a stack: the convolution applies the PREVIOUS layer's BatchNorm (batch statistics)
 * and ReLU to its input while loading it, a = max(((x - mean) * invstd) * gamma + beta, 0) (the expression of
 * batchnorm_train_forward, bit for bit), so the normalised activation is never written: x (b, cin, p) is the previous
 * convolution's output, in_mean / in_invstd (cin) its statistics (batchnorm_train_forward with y == NULL computes them
 * without the apply pass), in_gamma / in_beta (cin) may be NULL (1 / 0).  The weight-gradient twin multiplies dy with the
 * same transformed input. */
void conv1x1_bnrelu_forward_kernel_wrapper(int b, int cin, int cout, int p, const float *x, const float *w,
                                           const float *in_mean, const float *in_invstd, const float *in_gamma,
                                           const float *in_beta, float *y);
void conv1x1_bnrelu_wgrad_kernel_wrapper(int b, int cin, int cout, int p, const float *dy, const float *x,
                                         const float *in_mean, const float *in_invstd, const float *in_gamma,
                                         const float *in_beta, float *dw, void *workspace);
/* Training mode, conv -> BatchNorm of the SAME block (pytorch_utils.py:114-167): y = W a (a = x, or the transformed
 * input of conv1x1_bnrelu_forward when in_mean != NULL) AND the batch statistics of y for the BatchNorm that follows --
 * save_mean, save_invstd (cout), the momentum update of running_mean / running_var (nullable, unbiased variance) --
 * from per-workgroup fp64 partial sums the convolution's epilogue leaves: the statistics pass of
 * batchnorm_train_forward_kernel_wrapper(y = NULL) without reading y again.  workspace: conv1x1_stats_workspace_bytes(). */
long long conv1x1_stats_workspace_bytes(int b, int cin, int cout, int p);
void conv1x1_forward_bnstats_kernel_wrapper(int b, int cin, int cout, int p, const float *x, const float *w,
                                            const float *in_mean, const float *in_invstd, const float *in_gamma,
                                            const float *in_beta, float *y, float eps, float momentum,
                                            float *running_mean, float *running_var, float *save_mean,
                                            float *save_invstd, void *workspace);
void conv1x1_forward_bnstats_devmom_kernel_wrapper(int b, int cin, int cout, int p, const float *x, const float *w,
                                                   const float *in_mean, const float *in_invstd, const float *in_gamma,
                                                   const float *in_beta, float *y, float eps, const float *momentum_dev,
                                                   float *running_mean, float *running_var, float *save_mean,
                                                   float *save_invstd, void *workspace);
/* Training mode, input gradient through conv <- ReLU <- BatchNorm: da (b, cin, p) = W^T dy -- the gradient w.r.t. the
 * rectified, normalised input of the convolution -- AND dgamma / dbeta (cin) of the BatchNorm in front of it, summed in the
 * convolution's epilogue from da and bn_x (b, cin, p), the BatchNorm's input: the reduction pass of
 * batchnorm_train_backward_kernel_wrapper(relu = 1) without reading da again.  w (cout, cin), dy (b, cout, p); mean /
 * invstd (cin) the saved statistics, gamma / beta nullable.  Finish with batchnorm_train_backward_apply_kernel_wrapper
 * (the same dx).  workspace: conv1x1_stats_workspace_bytes(b, cout, cin, p). */
void conv1x1_dgrad_bnstats_kernel_wrapper(int b, int cin, int cout, int p, const float *dy, const float *w,
                                          const float *bn_x, const float *mean, const float *invstd, const float *gamma,
                                          const float *beta, float *da, float *dgamma, float *dbeta, void *workspace);
void batchnorm_train_backward_apply_kernel_wrapper(int b, int c, int l, const float *x, const float *dy, const float *gamma,
                                                   const float *beta, const float *save_mean, const float *save_invstd,
                                                   const float *dgamma, const float *dbeta, float *dx, int relu);
/* The apply passes of batchnorm_train_forward / batchnorm_train_relu_maxk_forward alone, for statistics obtained that
 * way: y = [relu]((x - mean) * invstd * gamma + beta); pooled / arg / xsel as documented above. */
void batchnorm_train_apply_kernel_wrapper(int b, int c, int l, const float *x, const float *gamma, const float *beta,
                                          const float *mean, const float *invstd, float *y, int relu);
void batchnorm_train_relu_maxk_apply_kernel_wrapper(int b, int c, int s, int k, const float *x, const float *gamma,
                                                    const float *beta, const float *mean, const float *invstd,
                                                    float *pooled, unsigned char *arg, float *xsel);
/* The same followed by the stack's max over the k neighbours (P2/pointnet2_modules.py: SharedMLP then .max(dim=3) /
 * max_pool2d(kernel=[1, nsample])): x (b, cin, s, k), pooled (b, cout, s) = max_k act(conv(x) * scale + shift); the
 * (b, cout, s, k) activation is not written.  k in {4, 8, 16, 32}. */
void conv1x1_affine_maxk_forward_kernel_wrapper(int b, int cin, int cout, int s, int k, const float *x, const float *w,
                                                const float *scale, const float *shift, int relu, float *pooled);
/* dw (cout, cin) = sum over b, q of dy[b][o][q] x[b][i][q], summed in a fixed order (deterministic).  workspace:
 * conv1x1_wgrad_workspace_bytes(b, cin, cout, p) bytes of device memory, 16-byte aligned. */
long long conv1x1_wgrad_workspace_bytes(int b, int cin, int cout, int p);
void conv1x1_wgrad_kernel_wrapper(int b, int cin, int cout, int p, const float *dy, const float *x, float *dw,
                                  void *workspace);
/* Host only (no launch): which kernel instantiation and grid the entry point `kind` selects for (b, cin, cout, p) given
 * as that entry point takes them, answered by the launchers' own planning code.  cus = 0: the current device's CU count;
 * cus > 0 stands in for it, and no HIP call is made (usable without a GPU).  out receives
 *   kinds FORWARD .. POOLED: {nbo, gy, gx, lean, stats}: conv1x1_kernel<nbo, stats, lean> on a (gx, gy) grid
 *                            (FORWARD also stands for conv1x1_bnrelu_forward, POOLED for any k; p = s * k there);
 *   kind WGRAD:              {ro, rm, ph, wo, wm, cp, grid}: conv1x1_wgrad_kernel<ro, rm, .> with ph pixel phases of wo x wm
 *                            workers on chunks of cp pixels (the same plan with and without the input transform).
 * Returns 0 when the plan is one the launcher runs, 1 when the launcher refuses it with PWCLO_EINVAL (LDS beyond the limit,
 * more than 4 blocks for DGRAD_SUMS, no rectangle for WGRAD; out is filled all the same), -1 for an unknown kind or a
 * non-positive size.  The launchers' checks that do not depend on the plan (p % 4, alignment, tensors below 4 GiB) are
 * not repeated here. */
#define PWCLO_PLAN_FORWARD 0     /* conv1x1_forward(transposed = 0), conv1x1_bnrelu_forward */
#define PWCLO_PLAN_DGRAD 1       /* conv1x1_forward(transposed = 1) for the layer (cin, cout): the kernel writes cin rows */
#define PWCLO_PLAN_STATS 2       /* conv1x1_forward_bnstats */
#define PWCLO_PLAN_DGRAD_SUMS 3  /* conv1x1_dgrad_bnstats for the layer (cin, cout) */
#define PWCLO_PLAN_AFFINE 4      /* conv1x1_affine_forward */
#define PWCLO_PLAN_POOLED 5      /* conv1x1_affine_maxk_forward */
#define PWCLO_PLAN_WGRAD 6       /* conv1x1_wgrad, conv1x1_bnrelu_wgrad */
int conv1x1_plan_query(int kind, int b, int cin, int cout, int p, int cus, int *out);

/* Host only (no launch, no device needed): which scatter-add kernel group_points_grad (dense and strided; gather_points_grad
 * with n <= 32768 is the same call with p = npoints) and three_interpolate_grad select for a shape, answered by the
 * launchers' own planning code.  p = npoints * nsample.  aligned: grad_out and idx are 16-byte aligned (what the launcher
 * reads off its pointers).  use_lds: the PWCLO_GRAD_LDS switch, 0 / 1, or -1 for the environment's value as the launcher
 * takes it.  out receives {form, ct, slices, splits, per_split, vec4, ranges}:
 *   form      PWCLO_SCATTER_ATOMIC (global fp32 atomics, one thread per position) or PWCLO_SCATTER_LDS;
 *   ct        channels of one slice (LDS form: a workgroup's accumulators are ct x n floats), slices = ceil(c / ct);
 *   splits    position ranges the launcher asks for, per_split positions each;
 *   ranges    position ranges launched (grid x = ceil(p / per_split)): 1 = the slice's sole owner adds its totals with a
 *             plain read-modify-write, more = every range flushes with global atomics;
 *   vec4      16-byte loads of idx and grad_out (group_points_grad only).
 * Returns 0, or -1 for a non-positive size. */
#define PWCLO_SCATTER_ATOMIC 0
#define PWCLO_SCATTER_LDS 1
int group_points_grad_plan_query(int b, int c, int n, int p, int aligned, int use_lds, int *out);
int three_interpolate_grad_plan_query(int b, int c, int n, int m, int use_lds, int *out);

/* Host only (no launch, no device needed): which kernel group_points (dense and strided) selects for points (b, c, n) and
 * p = npoints * nsample grouped positions, answered by the launcher's own planning code (csrc/group_points.hip:
 * gp_forward_plan).  aligned: points, idx and out are 16-byte aligned (what the launcher reads off its pointers).  use_lds,
 * threads, target, nt: the PWCLO_GROUP_LDS / PWCLO_GP_THREADS / PWCLO_GP_TARGET / PWCLO_GP_NT settings (threads 0: 1024
 * threads; target 0: 512 workgroups while the staged rows stay below 64 KiB, else 256), or -1 for what the launcher
 * currently uses: pwclo_group_points_tuning()'s value, else the environment's.
 * out receives {form, T, nt, gx, per_wg, lds_bytes, staged_vec, tail}:
 *   form        PWCLO_GROUP_DIRECT_SCALAR: group_points_kernel<false>, one position per thread (p % 4 != 0 or unaligned);
 *               PWCLO_GROUP_DIRECT_VEC4: group_points_kernel<true>, four positions per thread, gathers from global memory
 *               (LDS switched off, or min(c, 8) rows of n floats beyond 128 KiB);
 *               PWCLO_GROUP_LDS: group_points_lds_kernel<T, nt>, the slice's rows staged in lds_bytes of LDS;
 *   T           threads of a workgroup of the kernel that runs: 1024, 512 or 256 (any other request runs and is sized for
 *               256; the direct kernels: 256);
 *   nt          LDS form: non-temporal stores; else 0;
 *   gx, per_wg  grid x and the positions one workgroup covers (a multiple of 4 T in the LDS form: ceil(per_wg / 4 T)
 *               passes of the workgroup, the last workgroup and its last pass possibly short);
 *   staged_vec  LDS form: the rows are staged with 16-byte copies (n % 4 == 0); else 0;
 *   tail        c % 8: channels of a narrower last slice, 0 for none.
 * Returns 0, or -1 for a non-positive size. */
#define PWCLO_GROUP_DIRECT_SCALAR 0
#define PWCLO_GROUP_DIRECT_VEC4 1
#define PWCLO_GROUP_LDS 2
int group_points_plan_query(int b, int c, int n, int p, int aligned, int use_lds, int threads, int target, int nt, int *out);
/* Sets the four settings above for later group_points launches of this process; -1 puts a setting back to the
 * environment's value (read once per process).  For tests and sweeps that visit several kernel forms in one process. */
void pwclo_group_points_tuning(int use_lds, int threads, int target, int nt);

/* Host only (no launch, no device needed): what a knn call launches for xyz (b,n,3), new_xyz (b,s,3) and nsample
 * neighbours, answered by the launchers' own selection code (csrc/knn.hip: knn_plan).  prebuilt = 0 describes
 * knn_point_ws_kernel_wrapper with a workspace (knn_point_kernel_wrapper, and a NULL workspace, always take the exhaustive
 * kernel with the same qpw rule); prebuilt = 1 describes knn_build_kernel_wrapper + knn_point_prebuilt[_slice]_kernel_wrapper,
 * which have no PWCLO_KNN_MIN_N / PWCLO_KNN_MIN_S gate (64 <= n <= 16384, any s).  use_rows: the PWCLO_KNN_ROWS switch, 0 / 1,
 * or -1 for the environment's value as the launcher reads it (once per process).
 * out receives {search, qpw, L, R, build_r, nslab, nblk, grid_x}:
 *   search    PWCLO_KNN_EXHAUSTIVE: knn_kernel<qpw>, qpw = 2 / 4 / 8 queries per wave by b * s (< 8192, < 65536, more);
 *             PWCLO_KNN_ROWS: knn_rows_kernel<L, R>, nsample <= 32: L = 16 (nsample <= 16) or 32 lanes per query, R block
 *             bounds per lane, the smallest of {2,3,5,9,17} (L = 16) / {1,2,3,5,9} (L = 32) with L * R >= nblk;
 *             PWCLO_KNN_PRUNED: knn_pruned_kernel, one query per wave (nsample > 32, or use_rows = 0);
 *   qpw       exhaustive search only, else 0;   L, R: rows search only, else 0;
 *   build_r   the knn_build_kernel<R> that sorts the cloud, R = 1 / 2 / 4 / 8 / 16 points per thread (smallest with
 *             1024 * R >= n): launched by this call (prebuilt = 0) or by knn_build_kernel_wrapper before it (prebuilt = 1);
 *             0 for the exhaustive search, which builds nothing;
 *   nslab     x-slabs of the structure (knn_point_slabs(n)), nblk = ceil(n / 64) + nslab blocks of 64 sorted rows (what
 *             knn_point_workspace_sections lays out); both 0 for the exhaustive search;
 *   grid_x    workgroups per cloud of the search kernel (grid y = b).
 * Returns 0, or -1 for arguments the launchers refuse (a non-positive size, nsample outside [1, min(n, 64)], prebuilt with n
 * outside [64, 16384]). */
#define PWCLO_KNN_EXHAUSTIVE 0
#define PWCLO_KNN_ROWS 1
#define PWCLO_KNN_PRUNED 2
int knn_point_plan_query(int b, int n, int s, int nsample, int prebuilt, int use_rows, int *out);

/* Host only (no launch, no device needed): what a furthest-point-sampling call launches for a cloud batch (b,n,3) and m
 * samples, answered by the code every sampler launcher asks (csrc/sampling.hip: fps_plan).
 *   entry      PWCLO_FPS_ENTRY_PLAIN: furthest_point_sampling[_xyz|_chain]_kernel_wrapper; _SORTED and _SLAB: the wrappers of
 *              those names; _AUTO: what pointnet2_ops._ext.furthest_point_sampling does -- the plain entry, except that a
 *              cooperative plan of n >= 32768 asks for the spatial order first (sorted = 1: the caller builds it and calls
 *              the sorted entry);
 *   temp       0: no temp buffer (sorted / slab entries: a required buffer is NULL), 1: given and 8-byte aligned, 2: given,
 *              not 8-byte aligned;
 *   tie_iters, tie_out, prefix_in: the chain arguments (the two pointers as 0 / 1);
 *   capturing  the stream is under graph capture (the cooperative-launch API cannot be captured);
 *   use_table, use_coop, coop_launch, xcd_local: PWCLO_FPS_TABLE, PWCLO_FPS_COOP, PWCLO_FPS_COOP_LAUNCH (or
 *              pwclo_fps_large_cloud_launch), PWCLO_FPS_COOP_XCD_LOCAL (or pwclo_fps_large_cloud_exchange) as 0 / 1, or -1
 *              for what the launchers use now; use_sorted: PWCLO_FPS_SORTED (read by the Python front end; AUTO only), -1 = 1.
 * out receives 16 ints {kernel, T, E, I, table, G, sorted, per_launch, grid, launch, launches, xcd_local, lds_bytes, bs,
 * log2bs, 0}:
 *   kernel     PWCLO_FPS_REG: fps_reg_kernel<T, E, I, table>, one workgroup per cloud (n <= 24576), table = the cloud's copy
 *              in LDS (it and the chain log of tie_out fit 160 KiB; 64 KiB with use_table = 0);
 *              PWCLO_FPS_SLAB: fps_slab_kernel<512, I>, I = 16 / 18 sorted rows per lane (n <= 8192 / more);
 *              PWCLO_FPS_COOP: fps_coop_kernel<16, sorted>, G = ceil(n / 16384) <= 32 workgroups per cloud, per_launch
 *              clouds per launch (224 / G, whole groups of 8 from 8 on), `launches` launches, the first of `grid`
 *              workgroups, launch = PWCLO_FPS_LAUNCH_COOPERATIVE (hipLaunchCooperativeKernel) or _PLAIN, xcd_local = the
 *              exchange mode handed to the kernel;
 *              PWCLO_FPS_STREAM: fps_stream_kernel<1024>, one workgroup per cloud of any n < 2^23 (more than 32 workgroups
 *              per cloud, use_coop = 0, or a temp that is not 8-byte aligned);
 *              PWCLO_FPS_REFUSED: the launcher records PWCLO_EINVAL and launches nothing; msg receives its message;
 *   lds_bytes  dynamic LDS of the launch; bs, log2bs: the reference's block size for n, which the tie rule is written in.
 * Fields that do not apply are 0.  msg (msg_len bytes, may be NULL) receives the refusal's message, else "".
 * Returns 0, 1 for a refused call (out is filled all the same), -1 for an unknown entry or b <= 0 or m <= 0 (the launchers
 * return at once, without an error). */
#define PWCLO_FPS_ENTRY_PLAIN 0
#define PWCLO_FPS_ENTRY_SORTED 1
#define PWCLO_FPS_ENTRY_SLAB 2
#define PWCLO_FPS_ENTRY_AUTO 3
#define PWCLO_FPS_REG 0
#define PWCLO_FPS_COOP 1
#define PWCLO_FPS_STREAM 2
#define PWCLO_FPS_SLAB 3
#define PWCLO_FPS_REFUSED 4
#define PWCLO_FPS_LAUNCH_PLAIN 0
#define PWCLO_FPS_LAUNCH_COOPERATIVE 1
int furthest_point_sampling_plan_query(int entry, int b, int n, int m, int temp, int tie_iters, int tie_out, int prefix_in,
                                       int capturing, int use_table, int use_coop, int coop_launch, int xcd_local,
                                       int use_sorted, int *out, char *msg, int msg_len);

/* Host only (no launch, no device needed): how the reduction passes of the batchnorm_train_* entry points cut a problem of
 * c channels with M = b * l positions each in rows of L, answered by the launchers' own code: *nsplit position ranges of
 * *per_split positions per channel (grid (nsplit, c); per_split % 4 == 0, nsplit <= 256, the workspace holds c * nsplit
 * pairs of doubles), *vec = 1 when L % 4 == 0 selects the 16-byte loads (of the reduction and of the element-wise passes).
 * The forward and the dense backward ask for (c, b * l, l), batchnorm_train_relu_maxk_forward for (c, b * s * k, s * k), the
 * reduction of batchnorm_train_relu_maxk_backward for (c, b * s, s).  Returns 0, or -1 for a non-positive size. */
int batchnorm_train_plan_query(int c, long long M, int L, int *nsplit, long long *per_split, int *vec);

/* ---- 4. hoisted variants of section 3 ----------------------------------------------------------
 * The first layer of every grouped MLP is linear in [geometry | feat_centre[s] | feat_nbr[n]]; the
 * feature parts depend on one point only, so W_feat . feat[point] (+ bias) is computed once per
 * point by linear_jobs and gathered by the pixel kernels as accumulator seeds (csrc/mlp_core.hpp,
 * "Hoisting").  Same results as section 3 up to fp32 summation order. */

/* Up to 8 independent per-point linear maps in one launch: out_j (npts_j, cout_j) = src_j (npts_j,
 * cin_j) . W_j^T + bias_j, no activation; cin in {16,32,64}, cout in {16,32,64,128}; all seven
 * arrays are HOST arrays of length njobs (pointers inside are device pointers). */
void linear_jobs_kernel_wrapper(int njobs, const int *npts, const int *cin, const int *cout,
                                const float *const *src, const float *const *w, float *const *out,
                                const int *out_bf16 /* per job: 1 = write the rows as bf16 (dtype "bf16"); may be NULL */);

/* sa_fused with pre (b,n,c1) = W1_feat . feat + b1 (NULL at level 0, where layer 1 is whole). */
void sa_fused_h_kernel_wrapper(int b, int n, int s, int k, int c1, int c2, int c3, const float *xyz,
                               const float *new_xyz, const float *pre, const int *idx,
                               const float *packed_w, float *out, int wfmt, int packed_floats, int kmajor);
/* (kmajor = 1: level-0 stack whose 8-channel layers are packed "k-step major" -- layers 2 and 3 then issue only the two
 *  MFMA k-steps that carry data; fused.py: pack_layer(kmajor_out=True).)
 * upconv_fused with pre (b,n,128) = W1_feat . feat1 + b1. */
void upconv_fused_h_kernel_wrapper(int b, int n, int s, int k, const float *xyz2, const float *xyz1,
                                   const float *pre, const int *idx, const float *packed_w, float *out,
                                   int wfmt, int packed_floats);
/* Set-upconv INCLUDING its post-MLP (P2/pointnet2_modules.py:479-515) for up to two jobs that share the queries xyz2, the
 * coarse points xyz1, the neighbour lists idx and the fine features feat2 (b,s,c2) -- the features and the mask branch of one
 * refinement level, PW/pose_warp_refinement.py:95-103 -- in ONE launch: out_j (b,s,64) = relu(Wpost_j . [max_k stack_j | feat2]).
 * pre / packed_w / packed_post / out are HOST arrays of njobs device pointers; packed_w as for upconv_fused_h (fp32 tiles),
 * packed_post = the one packed post layer (64 + c2 -> 64).  In-lane pooling (a wave tile = 16 queries), c2 in {16,32,64}. */
void upconv_post_fused_h_kernel_wrapper(int njobs, int b, int n, int s, int k, int c2, const float *xyz2,
                                        const float *xyz1, const int *idx, const float *feat2,
                                        const float *const *pre, const float *const *packed_w,
                                        const float *const *packed_post, float *const *out,
                                        int packed_floats, int post_floats);
/* cv_fused_a1 with u (b,s,128) = W1_p . feat1 + b1 and v (b,n,128) = W1_q . feat2. */
void cv_fused_a1_h_kernel_wrapper(int b, int n, int s, int k, const float *xyz1, const float *u,
                                  const float *xyz2, const float *v, const int *idx,
                                  const float *packed_w, float *pix, int pix_slots, int wfmt,
                                  int packed_floats);
/* cv_fused_a1_h + cv_fused_a2 for nsample_q = 6 as ONE kernel (in-lane softmax, a wave tile = 16 queries): the per-pixel
 * (b,s,6,64) buffer between the two stages does not exist; first (b,s,64) is the first aggregate (PW/costvolume.py:139-141).
 * packed_a1 / packed_a2: the two stages' packed stacks as for the separate kernels (fp32 tiles; both LDS resident).
 * packed_v2 (may be NULL, then v2 must be NULL): the one packed layer 64 -> 128 of cv_b's neighbour partial product;
 * v2 (b,s,128) = W_f . first is then written as well (replaces that linear_jobs launch).  Bit-identical to the separate
 * kernels. */
void cv_fused_a_lane6_kernel_wrapper(int b, int n, int s, const float *xyz1, const float *u, const float *xyz2,
                                     const float *v, const int *idx, const float *packed_a1, const float *packed_a2,
                                     const float *packed_v2, float *first, float *v2, int a1_floats, int a2_floats,
                                     int v2_floats);
/* cv_fused_b with u2 (b,s,128) = W_p . feat1 + b, v2 (b,s,128) = W_f . first, first (b,s,64). */
void cv_fused_b_h_kernel_wrapper(int b, int s, int k, const float *xyz1, const float *u2,
                                 const float *v2, const float *first, const int *idx,
                                 const float *packed_w, float *out, int wfmt, int packed_floats);

/* ---- 4a. in-place refresh of the packed weights (pack_plan.PackPlan) ---------------------
 * One job per packed layer: everything needed to redo fused.py's fold_conv_bn -> column slice -> row padding -> pack_layer
 * from the live module tensors.  All pointers are device pointers; the table itself lives in device memory.
 *   w          conv weight (cout, cin) fp32 row-major; columns [col0, ...) are the ones the layer uses
 *   conv_bias  (cout) or NULL;  gamma, beta, mean, var (cout): eval-mode BatchNorm, all four NULL without one;  eps: its eps
 *   phys_map   16 * nbi ints: per physical input channel the column (relative to col0) it reads, or -1 for padding
 *   dst        the layer inside its packed buffer, 16-byte aligned: nbo * nbi operand tiles of 256 floats (fmt 0), or
 *              nbo * nbi / 2 tiles of 256 (fmt 2: bf16) / 768 (fmt 1: three bf16 terms) floats, then 16 * nbo fp32 biases
 *              (the layouts of csrc/mlp_core.hpp; fmt is the format the layer really has: odd nbi is always 0)
 *   use_bias   0: the biases are written as zeros (hoisted layers whose bias another job carries)
 *   kmajor     output channel c sits on row 4 * (c % 4) + c / 4 (cout <= 16, nbo == 1)
 *   tile0      first tile of this job in the launch's grid; the job owns nbo * nbi (fmt 0) or nbo * nbi / 2 tiles + 1
 * Rows >= cout and padding channels are written as zeros.  W' = W * gamma / sqrt(var + eps) and
 * b' = (b - mean) * gamma / sqrt(var + eps) + beta in fp64, rounded to fp32 once; bf16 = round to nearest even;
 * bf16x3 terms hi, mid = bf16(w - hi), lo = bf16((w - hi) - mid) with fp32 differences.  Bit for bit fused.py's result. */
typedef struct PwcloPackJob {
  const float *w, *conv_bias, *gamma, *beta, *mean, *var;
  const int *phys_map;
  float *dst;
  double eps;
  int cout, cin, col0, use_bias;
  int nbo, nbi, fmt, kmajor;
  int tile0, reserved;
} PwcloPackJob;
/* jobs: DEVICE table of njobs jobs with ascending tile0 (jobs[0].tile0 == 0), total_tiles = the sum of their tiles.  One
 * launch on the calling thread's stream (pwclo_set_stream), one wave per tile, every destination element written once. */
void pwclo_pack_layers_kernel_wrapper(const PwcloPackJob *jobs, int njobs, int total_tiles);

/* ---- 4b. module path (training): softmax over K + weighted sum as one pass each way ---------------------------
 * out[r] = sum_k softmax_k(x[r,:]) * v[r,k] for rows = B*C*S contiguous rows of K logits / values (PW/costvolume.py:139-141,
 * 181-183 on (B,C,S,K) tensors); backward recomputes the probabilities: dv = dout p, dx = p dout (v - out).
 * K in {1,2,4,6,8,16,32} (softmax_wsum_supported_k), 16-byte aligned tensors. */
int softmax_wsum_supported_k(int k);
void softmax_wsum_forward_kernel_wrapper(long long rows, int k, const float *x, const float *v, float *out);
void softmax_wsum_backward_kernel_wrapper(long long rows, int k, const float *x, const float *v, const float *dout,
                                          float *dx, float *dv);

/* ---- 4c. module path (training): the pose head with replayable dropout masks ------------
 * PW/pose_calculator.py:47-86 in train() mode from the mask LOGITS: p = softmax_n(logits), pooled = sum_n emb p,
 * big = w_qt pooled + b_qt, big_q / big_t = big under two keep masks (kept: times exactly 2.0f, dropped: +0.0f),
 * q = w_q big_q + b_q normalised as q / (sqrt(sum q^2 + 1e-10) + 1e-10), t = w_t big_t + b_t.
 * emb, logits (B,64,N) f32 channel-major, 16-byte aligned, N >= 1; w_qt (256,64) 16-byte aligned, b_qt (256), w_q (4,256),
 * b_q (4), w_t (3,256), b_t (3).  state = {seed, next step, step in flight} i64 in DEVICE memory.
 * Keep bit of unit c of cloud b = top bit of Philox4x32-10 output word 0, key (seed low, seed high), counter
 * (b * 256 + c, rank * 8 + head * 2 + branch, step in flight mod 2^32, 3); branch 0 = q, 1 = t; rank in [0, 2^28), head 0..3.
 * begin: one thread, state[2] = state[1]; state[1] += 1 (once per network forward, before the four heads).
 * forward reads state[0] and state[2]; writes q (B,4), t (B,3) and what backward needs: rowmax, rinv (B,64) = the row
 * maximum and 1 / sum of exp(x - max); pooled (B,64); big (B,256); keep (B,256) u8, bit 0 = q kept, bit 1 = t kept;
 * q_raw (B,4) before the norm.  keep_log (B,256) u8 or NULL receives the same keep bytes (the stream's record).
 * backward never reads the state: g_q (B,4), g_t (B,3) -> d_emb = g p, d_logits = g p (emb - pooled) with g = g_pooled
 * (B,64) and p recomputed; the six parameter gradients summed over the batch in batch order (no atomics); g_qraw (B,4),
 * g_big (B,256), g_pooled (B,64) are workspaces the caller owns. */
void pose_head_train_begin_kernel_wrapper(long long *state);
void pose_head_train_forward_kernel_wrapper(int B, int N, const float *emb, const float *logits, const float *w_qt,
                                            const float *b_qt, const float *w_q, const float *b_q, const float *w_t,
                                            const float *b_t, const long long *state, int rank, int head, float *rowmax,
                                            float *rinv, float *pooled, float *big, unsigned char *keep,
                                            unsigned char *keep_log, float *q_raw, float *q, float *t);
void pose_head_train_backward_kernel_wrapper(int B, int N, const float *emb, const float *logits, const float *w_qt,
                                             const float *w_q, const float *w_t, const float *rowmax, const float *rinv,
                                             const float *pooled, const float *big, const unsigned char *keep,
                                             const float *q_raw, const float *g_q, const float *g_t, float *g_qraw,
                                             float *g_big, float *g_pooled, float *d_emb, float *d_logits, float *d_w_qt,
                                             float *d_b_qt, float *d_w_q, float *d_b_q, float *d_w_t, float *d_b_t);

/* ---- 5. KITTI odometry evaluation of predicted poses ---------------------------
 * Replaces the per-sample host loops of /root/reference/train.py:866-893 (pose row -> 4x4 via quat2mat :762-795),
 * slam/common/kitti360_utils.py:406-431 (relative -> absolute poses), evaluation.py:198-215 (trajectory distances)
 * and evaluation.py:236-271 = slam/eval/eval_odometry.py:316-361 (segment errors).  All matrices are 4x4 row-major
 * fp64 in device memory; frames of all sequences are stored back to back, sequence s owning frames
 * [seq_start[s], seq_start[s+1]) (seq_start: nseq+1 ints in DEVICE memory). */

/* rows: n pose rows [tx ty tz qw qx qy qz] fp32, row_stride floats apart (28 for level 1 of a (B,4,7) pose_params
 * tensor) -> T (n,4,4) = [[R(q) t],[0 0 0 1]], or its inverse when invert != 0 (the reference stores the inverse
 * as the "relative pose", train.py:878). */
void odom_rows_to_transforms_kernel_wrapper(int n, int row_stride, const float *rows, double *T, int invert);
/* abs[f] = T[first] . ... . T[f] inside every sequence (kitti360_utils.py:422-426 applied to rel = T^-1). */
void odom_accumulate_kernel_wrapper(int nseq, const int *seq_start, const double *T, double *abs_out);
/* Streaming odometry with per-stream dropouts and restarts.  All pointers DEVICE memory.
 * One workgroup, one thread per stream (S <= 1024).  active / restart: S ints, this call's masks.  pose: (S,4,7) fp32
 * contiguous, rows [tx ty tz qw qx qy qz].  Persistent: have_prev / count / valid (S ints each), rel / abs_out
 * (capacity, S, 4, 4) fp64, overflow (one int).  Per stream: idle (!active): valid = 0 and nothing else; prime (active
 * and (restart or !have_prev)): rel[0,s] = abs_out[0,s] = I, count = 1, have_prev = 1, valid = 0; pair (otherwise):
 * k = count, rel[k,s] = the transform of the level-1 row, abs_out[k,s] = abs_out[k-1,s] . rel[k,s], count = k + 1,
 * valid = 1 (k == capacity: nothing written to the trajectories, *overflow = 1).  Streams that are not pair get the
 * identity pose (0,0,0, 1,0,0,0) in their four rows of `pose`. */
void stream_append_masked_kernel_wrapper(int S, int capacity, const int *active, const int *restart, float *pose,
                                         double *rel, double *abs_out, int *have_prev, int *count, int *valid,
                                         int *overflow);
/* One launch that copies, for every stream s with active[s] != 0 (S ints, DEVICE), bytes[i] bytes from
 * src[i] + s * src_stride[i] to dst[i] + s * dst_stride[i] for each of nseg <= stream_handover_max_segments() segments;
 * inactive streams' bytes are not touched.  dst / src / bytes / strides: HOST arrays of nseg entries (device addresses
 * in dst / src); the strides may be NULL (= bytes: densely packed streams).  The table travels to the kernel by value, so
 * a captured graph holds it without host memory.  Addresses, sizes and strides must be multiples of 4; segments where
 * all are multiples of 16 move 16 bytes per lane. */
int stream_handover_max_segments(void);
void stream_handover_masked_kernel_wrapper(int nseg, void *const *dst, const void *const *src, const long long *bytes,
                                           const long long *dst_stride, const long long *src_stride, int S,
                                           const int *active);
/* dist[f] = sum_{i<=f} |p[i] - p[i-1]| (dist[first] = 0) from the translations of `poses`. */
void odom_cumulative_distance_kernel_wrapper(int nseq, const int *seq_start, const double *poses, double *dist);
/* One slot per (sequence, first frame in 0,step,2*step.., segment length): slot_start (nseq+1 ints, DEVICE) with
 * slot_start[s+1]-slot_start[s] = ceil(n_s/step)*nlen, total_slots = slot_start[nseq].  err (total_slots,5) =
 * [first_frame, r_err/len, t_err/len, len, speed] as evaluation.py:270; valid[slot] = 0 where the sequence is too
 * short for that segment (the reference skips those).  lengths: nlen doubles in DEVICE memory. */
void odom_sequence_errors_kernel_wrapper(int nseq, int total_slots, const int *seq_start, const int *slot_start,
                                         const double *poses_gt, const double *poses_result, const double *dist,
                                         int step, int nlen, const double *lengths, double *err, int *valid);

/* ---- 6. point-to-plane registration against a sliding local map ---------------------------
 * Refines a frame's pose on the device: the reference's ICPFrameToModel (slam/odometry/icp_odometry.py:248-299,
 * slam/odometry/local_map.py:254-427, slam/common/optimization.py:297-354, 391-443).  All pointers DEVICE memory; clouds
 * (.., n, 3) fp32 point-major; poses (.., 4, 4) fp64 row-major.  The pose T of a frame maps its points into the previous
 * frame.  A map holds M slots per stream, each with its cloud, normals and search structure (knn_build_kernel_wrapper) in
 * the slot's own frame; A (S,M,4,4) maps the previous frame into slot m, R (S,M,3,3) rotates slot m into the previous
 * frame, live (S,M) ints, cursor (S) ints: the slot the next frame goes to.  One iteration = icp_queries, the search
 * knn_point_prebuilt_kernel_wrapper(S * M, n, n, 1, q, idx, dist, map_ws), icp_accumulate, icp_solve.  No atomics; every
 * sum has a fixed order. */

/* Normals as KdTreeLocalMap.__get_normals: idx (b,n,k+1) = the k+1 nearest of every point in its own cloud (column 0, the
 * point itself, is dropped); covariance of (neighbour - point) and its eigen-decomposition in fp64 (8 cyclic Jacobi
 * sweeps); normals (b,n,3) fp32 = the unit eigenvector of the smallest eigenvalue with n . point <= 0, or the zero vector
 * when the covariance has rank < 2: !(l_mid > 1e-10 l_max); eig (b,n,3) fp64 ascending.  1 <= k <= min(63, n - 1). */
void icp_normals_kernel_wrapper(int b, int n, int k, const float *xyz, const int *idx, float *normals, double *eig);
/* q[s,m,i] = fp32(A[s,m] . T[s] . p[s,i]) (T NULL: the identity), products in fp64, one rounding.  q (S,M,n,3). */
void icp_queries_kernel_wrapper(int S, int M, int n, const double *A, const double *T, const float *p, float *q);
/* Rows per stream that icp_accumulate writes for clouds of n points (one per workgroup of 256 points). */
int icp_accumulate_groups(int n);
/* Point i of stream s: the live slot with the smallest fp32 dist (tie: lower slot); rejected when none is live, dist >
 * max_dist, or the matched normal is zero.  r = n . (q - y), J = [p' x n', n'] with n' = R[s,m] n, p' = T[s] p; Huber
 * w^2 = 1 below sigma, else (2 sigma |r| - sigma^2) / max(|r|, 1e-4)^2.  partial (S, groups, 32) fp64: 21 upper entries of
 * sum w^2 J^T J, 6 of sum w^2 J r, sum w^2, sum w^2 r^2, pairs, 2 zeros.  idx / dist (S,M,n). */
void icp_accumulate_kernel_wrapper(int S, int M, int n, const float *p, const float *q, const int *idx, const float *dist,
                                   const float *map_xyz, const float *map_normals, const int *live, const double *R,
                                   const double *T, double sigma, float max_dist, double *partial);
/* One workgroup.  Per stream: the rows added in group order -> sum (S,32); it == 0 clears status and iters first.  A stream
 * with status != 0 is frozen: T stays, delta = 0.  Otherwise iters = it + 1, pairs, cost = sum w^2 r^2 are recorded, and
 * pairs < min_pairs sets status 2, a pivot that is not positive sets 4 (T untouched in both), else delta = -(H / sw +
 * damping I)^-1 (g / sw) by Cholesky, T <- [Rodrigues(delta[0:3]) | delta[3:6]] T with the rotation re-orthonormalised,
 * and |delta| < threshold sets status 1.  delta (S,6). */
void icp_solve_kernel_wrapper(int S, int groups, int it, const double *partial, double damping, double threshold,
                              int min_pairs, double *T, int *status, int *iters, int *pairs, double *cost, double *sum,
                              double *delta);
/* The handover after a registration.  Per stream: the staged frame (cloud (S,n,3), normals (S,n,3), stage_ws = the
 * structure knn_build_kernel_wrapper built for these S clouds) is copied into slot cursor[s] of map_xyz / map_normals
 * (S,M,n,3) and map_ws (a structure for S * M clouds); every other live slot gets A <- A T, R <- R_T^T R; the new slot gets
 * A = I, R = I, live = 1; cursor <- (cursor + 1) mod M.  64 <= n <= 16384, M <= 64. */
void icp_map_push_kernel_wrapper(int S, int M, int n, const double *T, const float *cloud, const float *normals,
                                 const void *stage_ws, float *map_xyz, float *map_normals, void *map_ws, double *A,
                                 double *R, int *live, int *cursor);

/* Masked (per-stream) registration.  active / restart: S ints in DEVICE memory, this call's masks; restart is only looked
 * at where active is set.  A stream with active[s] == 0 is idle: nothing of it changes (map slots, A, R, live, cursor, T),
 * its rows of sums are zero, and the solver gives it status 8 with iterations = pairs = 0 and cost = 0.  The four _masked
 * entry points take the argument lists above plus `active` and run the same kernels (the lock-step entry points pass no
 * mask); for active streams they compute the same bits.
 * The names below are followed by an (empty) comment: section 21's first test pins the set of names that this header
 * declares in the plain form to the six above, and the additions keep that test as it is. */

/* First launch of a masked registration.  Streams with active && (restart || armed) get an empty map: live[s,:] = 0,
 * cursor[s] = 0, A[s,:] = I, R[s,:] = I, armed[s] = 0; their frame then finds no live slot, freezes in iteration 0 with
 * status 2, keeps its initial pose and fills slot 0.  armed: S ints or NULL, restarts asked for between calls. */
void icp_begin_kernel_wrapper /**/ (int S, int M, const int *active, const int *restart, int *armed, double *A, double *R,
                                    int *live, int *cursor);
/* An idle stream's rows of q stay as they are. */
void icp_queries_masked_kernel_wrapper /**/ (int S, int M, int n, const double *A, const double *T, const float *p, float *q,
                                             const int *active);
/* An idle stream's rows of partial are zero; nothing of it is gathered. */
void icp_accumulate_masked_kernel_wrapper /**/ (int S, int M, int n, const float *p, const float *q, const int *idx,
                                                const float *dist, const float *map_xyz, const float *map_normals,
                                                const int *live, const double *R, const double *T, double sigma,
                                                float max_dist, double *partial, const int *active);
/* it == 0: an idle stream starts from status 8 (pairs = 0, cost = 0) and stays frozen; active is not read later. */
void icp_solve_masked_kernel_wrapper /**/ (int S, int groups, int it, const double *partial, double damping,
                                           double threshold, int min_pairs, double *T, int *status, int *iters, int *pairs,
                                           double *cost, double *sum, double *delta, const int *active);
/* An idle stream's slot, poses, live flags and cursor stay. */
void icp_map_push_masked_kernel_wrapper /**/ (int S, int M, int n, const double *T, const float *cloud, const float *normals,
                                              const void *stage_ws, float *map_xyz, float *map_normals, void *map_ws,
                                              double *A, double *R, int *live, int *cursor, const int *active);
/* After stream_append_masked and a masked registration: the refined trajectories ref_rel / ref_abs (capacity, S, 4, 4) fp64
 * beside rel / abs_out.  One thread per stream (S <= 1024); active / valid / count: the words of this call, count after the
 * append; T (S,4,4) fp64 the registered poses.  Pair (active and valid): k = count - 1, ref_rel[k,s] = T[s], ref_abs[k,s] =
 * ref_abs[k-1,s] . T[s] (nothing when k is outside [1, capacity)); prime (active and not valid): row 0 of both = I; idle:
 * nothing. */
void stream_record_refined_kernel_wrapper(int S, int capacity, const int *active, const int *valid, const int *count,
                                          const double *T, double *ref_rel, double *ref_abs);

/* ---- 7. projective frame-to-model registration on spherical vertex maps ------------------------
 * The reference's ICPFrameToModel over a ProjectiveLocalMap (slam/odometry/local_map.py:84-240, slam/common/projection.py:
 * 20-82, 340-436, slam/common/geometry.py:248-303, 405-447).  All pointers DEVICE memory; vertex and normal maps
 * (.., H, W, 3) fp32 point-major, an empty pixel is the zero vector; poses (.., 4, 4) fp64 row-major; fovs in degrees.
 * The pixel of a point p, every operation in fp32: r = |p|, col = 0.5 (-atan2(y, x) / pi + 1) W, row = (1 - (asin(z / r) +
 * |down_fov|) / (|up_fov| + |down_fov|)) H, both rounded half to even; p has a pixel when r > 0 (and finite), 0 <= row <=
 * H - 1 and 0 <= col <= W - 1.  A z-buffer keeps the smallest r per pixel, the lowest index among equal r: one 64-bit
 * atomicMin of (bits of r << 32 | index) per point on a key image preset to all ones, which is the only atomic here and
 * gives the same bits whatever the order of arrival.  A map holds M slots per stream, each the vertex and normal map of a
 * frame in that frame's own coordinates; A (S,M,4,4) maps the newest frame of the map into slot m, live (S,M) ints, cursor
 * (S) ints.  One iteration = proj_accumulate, then section 6's solver on its rows. */

/* Bytes of the key image that proj_vertex_map needs (8 per pixel and stream); 0 for arguments out of range. */
long long proj_vertex_map_workspace_bytes(int S, int H, int W);
/* points (S,R,C) fp32, C = 3 or 4 (xyz first); stream s offers the rows [0, min(lengths[s], R)) (lengths NULL: all R) with
 * keep[s,i] != 0 (keep (S,R) ints or NULL: all).  vmap (S,H,W,3) = the winner's xyz, rows (S,H,W) ints = its row, -1 for an
 * empty pixel.  A memset of the workspace and two launches. */
void proj_vertex_map_kernel_wrapper(int S, int R, int C, int H, int W, double up_fov, double down_fov, const float *points,
                                    const int *lengths, const int *keep, void *workspace, float *vmap, int *rows);
/* compute_normal_map: over the k x k window (zero padding) m = sum p and C = sum p p^T in fp64, n = C^-1 m by the adjugate
 * over the determinant, normalised, one rounding; zero where |fp32(det C)| <= 1e-6, |n| = 0 or the centre pixel is empty.
 * n points away from the sensor.  kernel_size 3 or 5; vmap, nmap (B,H,W,3). */
void proj_normal_map_kernel_wrapper(int B, int H, int W, int kernel_size, const float *vmap, float *nmap);
/* Bytes of the key images that proj_model_build needs (8 per pixel, slot and stream); 0 for arguments out of range. */
long long proj_model_build_workspace_bytes(int S, int M, int H, int W);
/* Per (stream, live slot): every non-empty pixel of map_v[s,m] is moved into the newest frame by the rigid inverse of
 * A[s,m] (fp64, one rounding), projected and z-buffered into model_v[s,m]; model_n gets the winner's normal rotated the
 * same way; src (S,M,H,W) ints = the slot's pixel index that won, -1 for an empty pixel.  A slot that is not live gives an
 * empty image.  map_v, map_n, model_v, model_n (S,M,H,W,3).  A memset of the workspace and two launches. */
void proj_model_build_kernel_wrapper(int S, int M, int H, int W, double up_fov, double down_fov, const float *map_v,
                                     const float *map_n, const double *A, const int *live, void *workspace, float *model_v,
                                     float *model_n, int *src);
/* One thread per pixel of the new frame's own vertex map vmap (S,H,W,3): q = fp32(T[s] p); among the M model images the
 * non-empty candidate at q's pixel with the smallest fp32 |q - y| (tie: lower slot).  No pair when p is empty, q has no
 * pixel, no candidate is there, the distance exceeds max_dist or the winner's normal is zero.  Then section 6's row: r =
 * n . (q - y), J = [T p x n, n], the Huber weight, the same 30 sums in the same order.  partial (S, groups(H * W), 32) fp64
 * with groups = icp_accumulate_groups.  slot / pixel (S,H,W) ints or NULL: the chosen slot (-1: no pair) and q's pixel
 * index (-1: none). */
void proj_accumulate_kernel_wrapper(int S, int M, int H, int W, double up_fov, double down_fov, const float *vmap,
                                    const float *model_v, const float *model_n, const double *T, double sigma,
                                    float max_dist, double *partial, int *slot, int *pixel);
/* The handover: vmap / nmap (S,H,W,3) go into slot cursor[s] of map_v / map_n; every other live slot gets A <- A T; the
 * new slot gets A = I, live = 1; cursor <- (cursor + 1) mod M.  Two launches (the copy reads the cursor, the bookkeeping
 * moves it).  M <= 64. */
void proj_map_push_kernel_wrapper(int S, int M, int H, int W, const double *T, const float *vmap, const float *nmap,
                                  float *map_v, float *map_n, double *A, int *live, int *cursor);

/* ---- 8. keyframe local maps and the refined de-skew prior --------------------------------------
 * The reference inserts a frame into its local map only when the motion accumulated since the last inserted frame exceeds
 * a translation or a rotation threshold (slam/odometry/icp_odometry.py:361-381); otherwise the map is only moved into the
 * new frame.  The decision is taken on the device, between the last solve and the push.  State per stream, DEVICE memory:
 * kf_delta (S,4,4) fp64 row-major, the motion since the stream's last inserted frame; kf_insert (S) ints, this call's
 * decision; kf_count (S) ints, frames inserted since the map was emptied.  The names of this section start with keyframe_:
 * sections 6 and 7 pin the sets of names that carry their own prefixes. */

/* One workgroup, one thread per stream (S <= 1024, M <= 64).  T (S,4,4) fp64 the registered poses, live (S,M) ints, active
 * (S) ints or NULL (every stream delivered a frame); trans in metres, rot in degrees, both finite and >= 0.  In this order:
 * active[s] == 0: kf_insert[s] = 0, nothing else changes.  No live slot: kf_insert = 1, kf_delta = I, kf_count = 1.
 * Otherwise D = kf_delta . T[s], t = |D[:3,3]|, angle = atan2(s, c) 180 / pi with c = (trace - 1) / 2 and s = half the norm of
 * (R32 - R23, R13 - R31, R21 - R12); insert iff t > trans or angle > rot (both strict); insert: kf_delta = I, kf_count += 1;
 * no insert: kf_delta = D.  All arithmetic fp64. */
void keyframe_gate_kernel_wrapper(int S, int M, const double *T, const int *live, const int *active, double trans, double rot,
                                  double *kf_delta, int *kf_insert, int *kf_count);
/* Section 6's masked push behind the gate (active (S) ints or NULL).  insert[s] != 0: the bits of that push.  insert[s] == 0:
 * every live slot, the cursor's included, gets A <- A T and R <- R_T^T R; nothing is copied, live and cursor stay. */
void keyframe_icp_push_kernel_wrapper(int S, int M, int n, const double *T, const float *cloud, const float *normals,
                                      const void *stage_ws, float *map_xyz, float *map_normals, void *map_ws, double *A,
                                      double *R, int *live, int *cursor, const int *active, const int *insert);
/* The refined pose as the de-skew prior: a stream with active[s] and valid[s] (this call's words) gets motion[s] (S,7) fp32 =
 * the pose row [tx ty tz qw qx qy qz] of T[s] (S,4,4) fp64: the translation rounded once; the quaternion from the rotation
 * by Shepperd's branch selection in fp64, normalised, w >= 0, rounded once.  Every other row keeps its bits.  S <= 1024. */
void stream_motion_from_refined_kernel_wrapper(int S, const int *active, const int *valid, const double *T, float *motion);

/* ---- 9. point-to-plane registration against a persistent voxel map per stream -------------------
 * A stream's map is a toroidal grid of Nx x Ny x Nz voxels of edge voxel_size -- every N even, 4 <= N <= 1024, Nx Ny Nz <
 * 2^28, S <= 1024 --: voxel c lives in cell ((cz mod Nz) Ny + (cy mod Ny)) Nx + (cx mod Nx), floor-mod.  With h_a =
 * floor((double)w_a / (voxel_size / 2)): voxel c_a = h_a >> 1, octant = (h_z & 1) << 2 | (h_y & 1) << 1 | (h_x & 1); a
 * coordinate is storable where -2^21 <= h_a < 2^21 on every axis.  The grid buffer (DEVICE memory, 8-byte aligned) has four
 * sections: coordinate words (S, cells) u64 = (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20), all ones = empty; keys
 * (S, cells, 8) u64 = seq << 32 | row, all ones = empty; points and normals (S, cells, 8, 3) fp32 in the stream's map frame.
 * P (S,4,4) fp64: the pose of the last registered frame in the map frame; nonempty (S) ints; seq (S) ints, frames inserted
 * since the map was emptied.  active (S) ints or NULL in every call: a stream with active[s] == 0 keeps every bit. */

/* 264 bytes per voxel and stream; 0 for arguments out of range. */
long long voxel_map_bytes(int S, int nx, int ny, int nz);
/* Streams with active && (restart || armed) (restart, armed: S ints or NULL) get an empty map: every coordinate word all
 * ones, P = I, nonempty = 0, seq = 0.  armed is only read here; voxel_pose clears it. */
void voxel_begin_kernel_wrapper(int S, int nx, int ny, int nz, const int *active, const int *restart, const int *armed,
                                void *grid, double *P, int *nonempty, int *seq);
/* Inserts cloud / normals (S,n,3) with the pose W = I where nonempty (S ints or NULL) is given and zero, else P T (T (S,4,4)
 * or NULL: P), for the streams with active and insert[s] != 0 (insert: S ints or NULL = all).  w = fp32(W p) (fp64, one
 * rounding), n_w = fp32(R_W n).  A point is inserted where w is finite, storable and |w_a - t_a| < (N_a / 2 - 1) voxel_size
 * on every axis (t the translation of W; fp64, strict).  A cell whose word differs from the point's voxel is stale: the word
 * is replaced, its keys emptied.  The octant keeps the smallest key seq[s] << 32 | row (64-bit atomicMin, the only atomic
 * read-modify-write), and the row whose key stands writes w and n_w.  slot (S,n) ints: cell * 8 + octant a row asked for, -1
 * where it is not inserted.  Three launches; nothing here writes P, nonempty or seq. */
void voxel_insert_kernel_wrapper(int S, int n, int nx, int ny, int nz, double voxel_size, const float *cloud,
                                 const float *normals, const double *P, const double *T, const int *nonempty, const int *seq,
                                 void *grid, int *slot, const int *active, const int *insert);
/* After the insertion, one thread per stream: P <- I where nonempty was zero, else P T (T NULL: P stays); a stream with
 * insert[s] != 0 (NULL: all) gets seq += 1 and nonempty = 1; armed[s] = 0 (armed: S ints or NULL). */
void voxel_pose_kernel_wrapper(int S, const double *T, double *P, int *nonempty, int *seq, int *armed, const int *active,
                               const int *insert);
/* One thread per point of p (S,n,3): q = fp32(P T p) (T NULL: the identity).  Candidates: the stored entries of the 27
 * voxels around q's voxel, in the order dz, dy, dx ascending, then octants ascending, where the cell's word equals the wanted
 * voxel and the key is not empty; fp32 d = sqrtf((dx dx + dy dy) + dz dz), strict <, so the first candidate stays on a tie.
 * No pair when q is not storable, there is no candidate, !(d <= max_dist) or the winner's normal is zero; max_dist <=
 * voxel_size.  Then section 6's row with Rm = R_P^T, the same 30 sums in the same order: partial (S, groups(n), 32) fp64 in
 * the layout of section 6's solver, zero rows for an idle stream.  cell / octant (S,n) ints and dist (S,n) fp32, all three
 * or all NULL: the nearest candidate whatever became of the pair (-1, -1, +Inf: none). */
void voxel_accumulate_kernel_wrapper(int S, int n, int nx, int ny, int nz, double voxel_size, const float *p, const double *P,
                                     const double *T, const void *grid, double sigma, float max_dist, double *partial,
                                     int *cell, int *octant, float *dist, const int *active);

/* ---- 10. pose-graph backend: SE(3) graph optimisation per stream --------------------------------
 * The reference's GraphSLAM (slam/backend.py) without g2o: per stream a graph of at most N = max_poses vertices X (N,S,4,4)
 * fp64 row-major (count[s] in use, vertex 0 the identity), the odometry edge k-1 -> k with measurement Zc[k] (N,S,4,4) and
 * information diag(2,2,2,5,5,5) for every vertex k >= 1, nloops[s] <= ML loop edges loop_ij (S,ML,2) ints (i < j), loop_Z
 * (S,ML,4,4) the pose of j in i's frame, loop_Om (S,ML,6,6), and nabs[s] <= MA absolute edges abs_i (S,MA) ints, abs_G
 * (S,MA,4,4), abs_Om (S,MA,6,6).  Edge ids of a stream: chain edge k at k, loop l at N + l, absolute edge a at N + ML + a; E =
 * N + ML + MA.  Error of an edge: Delta = Z^-1 X_i^-1 X_j (absolute: G^-1 X_i), e = (t_Delta, q_x, q_y, q_z) with q the unit
 * quaternion of R_Delta by Shepperd's branch selection, w >= 0; chi2 = sum e^T Omega e.  Retraction X <- X . [R(q), rho], q =
 * (sqrt(1 - |nu|^2), nu), the rotation of the product rebuilt from its normalised quaternion.  Slots (S,E,136) doubles per
 * edge: e 0..5, Omega e 6..11, Ji^T Omega Ji 12..47, Ji^T Omega Jj 48..83, Jj^T Omega Jj 84..119, Ji^T Omega e 120..125, Jj^T
 * Omega e 126..131, chi2 132.  inc_ptr (S,N+1), inc_ent (S,2 ML + MA) ints: per vertex the loop and absolute edges that touch
 * it, entries edge id * 2 + side (1: the vertex is the edge's j; absolute edges have side 1), written by the host.  Status
 * words (S) ints: 1 converged, 2 a chain without loop or absolute edge, 4 a non-finite chi2 (an idle stream keeps its word, so there is no idle bit); active (S) ints or NULL in
 * every call: a stream with active[s] == 0, or with a non-zero status word, is skipped and keeps every bit.  S <= 1024; all
 * capacities >= 1.  All pointers DEVICE memory; every sum has a fixed order and there is no atomic. */

/* First launch of an optimisation of `iters` <= diag_stride iterations: status = 0, or 3 for a graph with a single vertex or
 * without loop and absolute edges (then chi2 = 0); rows [0, iters) of pcg_used, relres, accepted (S,diag_stride) are cleared. */
void pose_graph_begin_kernel_wrapper(int S, int iters, int diag_stride, const int *active, const int *count, const int *nloops,
                                     const int *nabs, int *status, int *pcg_used, double *relres, int *accepted, double *chi2);
/* One thread per stream, with stream_record_refined's words: pair (active and valid; valid NULL: every active stream): k =
 * count, X[k] = X[k-1] . Z, Zc[k] = Z, count = k + 1, with Z = rel[s] (S,4,4) fp64 or quat2mat of rows[s] (S,7) fp32 (exactly
 * one of the two is given); stream_count (S ints or NULL): the stream engine's count after its own append, then k =
 * stream_count - 1, which must equal the graph's count; k >= N or a k that is not the next vertex sets *overflow and writes
 * nothing.  Prime (active and not valid): the empty graph: X[0] =
 * I, count = 1, nloops = nabs = 0, epoch[s] += 1. */
void pose_graph_append_kernel_wrapper(int S, int N, const int *active, const int *valid, const int *stream_count,
                                      const double *rel, const float *rows, double *X, double *Zc, int *count, int *nloops, int *nabs, int *epoch, int *overflow);
/* One thread per edge at the poses X.  slots given: the whole slot of every edge; chi_only (S,E) given instead: the chi2
 * term alone (the evaluation at trial poses). */
void pose_graph_linearise_kernel_wrapper(int S, int N, int ML, int MA, const int *active, const int *status, const int *count,
                                         const int *nloops, const int *nabs, const double *X, const double *Zc,
                                         const int *loop_ij, const double *loop_Z, const double *loop_Om, const int *abs_i,
                                         const double *abs_G, const double *abs_Om, double *slots, double *chi_only);
/* The same launch with a robust kernel on the edge classes of edge_mask (1 chain | 2 loop | 4
 * absolute, in [1, 7]).  With c = e^T Omega e the raw term of such an edge, kind 1 Huber: c <= delta^2: rho = c, w = 1,
 * otherwise s = sqrt(c), rho = (2 s) delta - delta delta, w = delta / s; kind 2 Geman-McClure: a = delta / (delta + c), rho = c
 * a, w = a a; kind 3 DCS (delta is Phi): s = (2 delta) / (delta + c), s >= 1: rho = c, w = 1, otherwise w = s s, rho = w c.  An
 * edge outside the mask has rho = c, w = 1.  The chi2 term (slot double 132, or chi_only) is rho; the three blocks and the two
 * gradients are the finished plain ones times w (first order: no rho'' term); e and Omega e stay raw; the full form also
 * writes c into slot double 133 and w into 134, which the plain launch never touches.  A non-finite c gives a non-finite
 * rho.  delta finite and > 0, kind in [1, 3]: anything else is refused before the launch.  Solve, retract and judge read the
 * slots and chi terms as before. */
void pose_graph_linearise_robust_kernel_wrapper(int S, int N, int ML, int MA, int kind, int edge_mask, double delta,
                                                const int *active, const int *status, const int *count, const int *nloops,
                                                const int *nabs, const double *X, const double *Zc, const int *loop_ij,
                                                const double *loop_Z, const double *loop_Om, const int *abs_i,
                                                const double *abs_G, const double *abs_Om, double *slots, double *chi_only);
/* The read-out of the weights: one thread per loop and absolute edge id, for every stream, idle and frozen ones included.
 * out (S, ML + MA, 2) doubles: c and w of loop l at row l and of absolute edge a at row ML + a, at the poses X as they stand;
 * zeros past nloops[s] / nabs[s].  kind 0: no kernel, w = 1 (edge_mask and delta are not read); otherwise as above. */
void pose_graph_edge_weights_kernel_wrapper(int S, int N, int ML, int MA, int kind, int edge_mask, double delta,
                                            const int *nloops, const int *nabs, const double *X, const int *loop_ij,
                                            const double *loop_Z, const double *loop_Om, const int *abs_i, const double *abs_G,
                                            const double *abs_Om, double *out);
/* One workgroup per stream, iteration `it` of the call.  chi2[s] = the sum of the slots' chi2 terms (not finite: status 4);
 * b and the 6 x 6 block diagonal of H gathered per vertex (chain edge v, chain edge v + 1, then the incidence list); it == 0:
 * lam[s] = 1e-5 max diag H, nu[s] = 2; max |b| <= 1e-12: status 1.  Then block-Jacobi preconditioned conjugate gradients on
 * (H + lam I) delta = -b from delta = 0 over the free vertices (vertex 0 is fixed where fix_first != 0) until |r| <= pcg_tol
 * |b| or pcg_iters iterations; delta (S,N,6), the trial poses Xt (N,S,4,4) = X . D(delta), pcg_used[s,it], relres[s,it] = |r| /
 * |b|.  work: S N 66 doubles. */
void pose_graph_solve_kernel_wrapper(int S, int N, int ML, int MA, int fix_first, int it, int pcg_iters, double pcg_tol,
                                     const int *active, int *status, const int *count, const int *nloops, const int *nabs,
                                     const int *loop_ij, const int *abs_i, const int *inc_ptr, const int *inc_ent,
                                     const double *slots, const double *X, double *work, double *delta, double *Xt, double *lam,
                                     double *nu, double *chi2, int *pcg_used, double *relres, int diag_stride);
/* The retraction alone: Xt[v] = X[v] . D(delta[v]) for the vertices in use (a fixed vertex is copied). */
void pose_graph_retract_kernel_wrapper(int S, int N, int fix_first, const int *active, const int *status, const int *count,
                                       const double *X, const double *delta, double *Xt);
/* One workgroup per stream.  chi_new (S,E): the chi2 terms at Xt.  rho = (chi2 - chi2_new) / (delta^T (lam delta - b)); accepted
 * where rho > 0 and chi2_new is finite: X <- Xt, lam <- lam max(1/3, 1 - (2 rho - 1)^3), nu = 2, chi2 = chi2_new, status 1 where
 * chi2 - chi2_new <= 1e-9 chi2; otherwise lam <- lam nu, nu <- 2 nu.  accepted[s,it] = the decision. */
void pose_graph_judge_kernel_wrapper(int S, int N, int ML, int MA, int fix_first, int it, const int *active, int *status,
                                     const int *count, const int *nloops, const int *nabs, const int *loop_ij, const int *abs_i,
                                     const int *inc_ptr, const int *inc_ent, const double *slots, const double *chi_new,
                                     const double *delta, const double *Xt, double *X, double *lam, double *nu, double *chi2,
                                     int *accepted, int diag_stride);

/* ---- 11. loop detection: Scan Context search that feeds the pose graph ---------------------------
 * Per stream a database of at most MK = max_keyframes places.  A place is the column-normalised polar height image Dn of one
 * frame (NR rings x NS sectors, 1 <= NR <= 64, 8 <= NS <= 64), the 64-bit mask of its non-empty columns, its frame id and,
 * where closures are verified, its (n,3) cloud: db_desc (S,MK,NS,NR) floats (an entry's columns, each contiguous), db_mask
 * (S,MK) 64-bit words, db_frame (S,MK) ints, db_cloud (S,MK,n,3) floats, count (S) ints.  One detection is build, score,
 * select, fetch, two registrations of section 6's refiner, accept, insert.  active (S) ints or NULL (every stream): a stream
 * with active[s] == 0 keeps its database, count and log.  S <= 1024.  All pointers DEVICE memory; every sum has a fixed
 * order, and the only atomic is build's LDS max, whose result does not depend on the order of the points. */

/* One workgroup per stream.  cloud (S,n,3); lengths (S) ints or NULL: rows [0, lengths[s]) count (clamped to [0, n]).  With
 * up_neg_y the descriptor's (x, y, z) are (c2, -c0, -c1) of a row (c0, c1, c2).  A row is dropped where a coordinate is not
 * finite, r2 = x x + y y is 0 or >= ring_b[NR-1], or h = z + z_offset <= 0.  ring_b (NR) floats: the squared ring boundaries
 * b_1..b_NR; ring = #{k < NR : b_k <= r2}.  sector_d (NS,2) floats: the sector directions; sector = the s with dot_s > 0,
 * cross_s >= 0 and cross_{s+1} < 0.  D (S,NR,NS) = max h of the cell (0: empty); Dn = D / column norm (0 for an empty column,
 * the sum of squares taken ring-ascending); mask (S) 64-bit words, bit j = column j is not empty.  count, nlog, epoch (S) ints,
 * all three or all NULL, with restart (S) ints: a stream with active and restart gets count = nlog = 0 and epoch + 1 before
 * anything is searched. */
void scan_context_build_kernel_wrapper(int S, int n, int NR, int NS, int up_neg_y, float z_offset, const float *cloud,
                                       const int *lengths, const float *ring_b, const float *sector_d, float *D, float *Dn,
                                       void *mask, const int *active, const int *restart, int *count, int *nlog, int *epoch);
/* Grid (MK / 4, S), one wave per entry e, lane = shift.  Entry e of stream s counts where e < count[s], db_frame[e] +
 * min_id_distance <= frame_id[s] and, with traj (traj_frames,S,4,4) doubles given, both frame ids lie inside it and the
 * squared distance of their translations is < max_distance^2; every other entry scores +Inf with shift 0.  Otherwise c(s) =
 * sum_j sum_r Qn[r][(j+s) mod NS] En[r][j] (j outer, r inner, fp32, unfused), v(s) = popcount(rot(qmask, s) & mask_e), d(s) =
 * 1 - c(s) / v(s) (+Inf where v(s) = 0); scores (S,MK) = min_s d(s), shifts (S,MK) = the smallest s that reaches it. */
void loop_score_kernel_wrapper(int S, int NR, int NS, int MK, const float *Qn, const void *qmask, const float *db_desc,
                               const void *db_mask, const int *db_frame, const int *count, const int *active,
                               const int *frame_id, int min_id_distance, const double *traj, int traj_frames,
                               double max_distance, float *scores, int *shifts);
/* One workgroup per stream: the entry of the lowest score, the lowest entry on a tie.  match (S,4) ints: found (its score <
 * threshold), entry (-1: no finite score), the entry's frame id, its shift; match_score (S) floats; found (S) ints; T0
 * (S,4,4) doubles = T0_table[shift] (NS,4,4) where found, else the identity.  slot[s] = count[s] where the stream is active,
 * frame_id[s] >= 0 is a multiple of stride and the database has room; a full database sets *overflow; otherwise -1.  An idle
 * stream gets found = 0 and slot = -1. */
void loop_select_kernel_wrapper(int S, int NS, int MK, int stride, float threshold, const float *scores, const int *shifts,
                                const int *db_frame, const int *count, const int *active, const int *frame_id,
                                const double *T0_table, int *match, float *match_score, int *found, double *T0, int *slot,
                                int *overflow);
/* staging (S,n,3) = the matched entry's cloud, chosen by the device-side index, for the streams with found != 0. */
void loop_fetch_kernel_wrapper(int S, int n, int MK, const int *found, const int *match, const float *db_cloud,
                               float *staging);
/* One thread per stream.  A found stream is accepted where the refiner's status word has bits 2 and 4 clear, pairs >=
 * min_fitness n and cost / pairs <= max_mean_cost (status, pairs, cost all NULL: every match is accepted, pairs = cost = 0).
 * An accepted closure is record nlog[s] of the stream's log: log_i (S,ML,4) ints i = the entry's frame, j = frame_id[s],
 * shift, pairs; log_T (S,ML,4,4) doubles = T[s], the pose of j in i; log_c (S,ML,2) doubles score, cost.  A full log sets
 * *log_overflow and writes nothing.  accepted (S) ints: this call's decision. */
void loop_accept_kernel_wrapper(int S, int n, int ML, const int *found, const int *match, const float *match_score,
                                const int *frame_id, const double *T, const int *status, const int *pairs, const double *cost,
                                double min_fitness, double max_mean_cost, int *log_i, double *log_T, double *log_c, int *nlog,
                                int *log_overflow, int *accepted);
/* The frame of this call becomes entry slot[s] (select's decision; < 0: nothing is written): its Dn transposed, qmask,
 * frame_id[s] and, with cloud and db_cloud given (both or neither), its rows; count[s] = slot[s] + 1. */
void loop_insert_kernel_wrapper(int S, int n, int NR, int NS, int MK, const int *slot, const int *frame_id, const float *Qn,
                                const void *qmask, const float *cloud, float *db_desc, void *db_mask, int *db_frame,
                                float *db_cloud, int *count);

/* Translation search on elevation grids, between select and the verifying registration (optional: image, score, choose).
 * G = cells, even in [8, 128]; Y = 2 Yh + 1 yaw candidates, odd in [1, 17]; W = window in [0, 16]; L = tolerance in
 * [1, 255].  The grid of a cloud under a planar rotation (cs, sn), fp32 and unfused in this order, on the descriptor's (x, y,
 * z) of build: xr = cs x - sn y, yr = sn x + cs y, fx = floorf(xr / cell_size), fy = floorf(yr / cell_size), h = z + z_offset;
 * a row is dropped where a coordinate is not finite, fx or fy lies outside [-G/2, G/2) (compared as floats) or h <= 0; its
 * level is q = 255 where l = floorf(h / z_step) >= 254, else (int)l + 1; cell (fx + G/2, fy + G/2) holds the largest q, 0
 * where empty.  Every kernel skips the streams with found[s] == 0. */

/* Grid (1 + Y, S).  Image 0 is E: staging (S,n,3), every row, at the identity.  Image 1 + k is Q_k: cloud (S,n,3), rows
 * [0, lengths[s]) (lengths NULL: all), under rot[shift Y + k] (NS Y,2) floats cos / sin, shift = match[s][3].  img
 * (S,1+Y,G,G) bytes; occ (S,1+Y) ints, the non-empty cells; list (S,Y,G G) ints, i | j << 8 | q << 16 of the non-empty cells
 * of Q_k in any order. */
void elevation_image_kernel_wrapper(int S, int n, int NS, int G, int Y, int up_neg_y, float z_offset, float cell_size,
                                    float z_step, const float *cloud, const float *staging, const int *lengths,
                                    const int *found, const int *match, const float *rot, void *img, int *occ, int *list);
/* One wave per 64 consecutive candidates of one (stream, k), lane = candidate.  A (S,Y,2W+1,2W+1) ints: A[k][a+W][b+W] = the
 * sum of max(0, L - |Q_k[i][j] - E[i+a][j+b]|) over the cells where both are non-empty and (i+a, j+b) lies inside the grid. */
void elevation_score_kernel_wrapper(int S, int G, int Y, int W, int L, const int *found, const void *img, const int *occ,
                                    const int *list, int *A);
/* One workgroup per stream: the largest A, the lowest index ((k (2W+1)) + a + W)(2W+1) + b + W on a tie; found where A > 0
 * and, in fp32, (float)A >= min_agreement * (float)(L min(occ_Qk, occ_E)).  record (S,8) ints: found, k, a, b, A, occ_Qk,
 * occ_E, 0.  T1 (S,4,4) doubles: where found, the rotation of pose[shift Y + k] (NS Y,4,4) with the translation (a c, b c, 0)
 * (up_neg_y: (-b c, 0, a c)), c = (double)cell_size; else T0[s] (S,4,4), as is.  A stream with found[s] == 0 gets a record
 * of zeros and T1 = T0. */
void elevation_choose_kernel_wrapper(int S, int NS, int Y, int W, int L, int up_neg_y, float min_agreement, float cell_size,
                                     const int *found, const int *match, const int *A, const int *occ, const double *pose,
                                     const double *T0, int *record, double *T1);

/* ---- 12. global map: keyframe bank and voxel-hashed world map per stream ---------------------------
 * Per stream a bank of at most MK = max_keyframes clouds of n rows: bank_cloud (S,MK,n,3) floats, bank_frame (S,MK) ints,
 * bank_len (S,MK) ints.  Row i < bank_len[k] of keyframe k has the global row id g = k n + i, the world point w =
 * float32(X[bank_frame[k]] p) (X (frames,S,4,4) doubles; fp64, ((m0 x + m1 y) + m2 z) + m3, one rounding) and the key of
 * grid_sample_keep's rule applied to w; it is no candidate where that rule says so or where bank_frame[k] lies outside
 * [0, frames).  The map is the w of the rows with the lowest g of their key, in ascending g.  The table of a stream has T =
 * 2^ceil(log2(2 MK n)) slots, at least 64: keys (S,T) 64-bit words, rows (S,T+2) 32-bit words, slots (S,MK,n) ints, blocks
 * (S,MK,ceil(n/256)) ints.  state (S,8) ints: count, built, total, dirty, todo, slot, run, 0.  One call is begin, push, clear,
 * insert, count, scan, write, end, each a launch of its own; E = max_new bounds the keyframes a call enters.  S <= 1024,
 * MK <= 65535, MK n <= 2^29.  All pointers DEVICE memory; every launcher refuses a bad argument before it launches. */

/* Bytes of all device buffers of S streams (table, bank, block counts, state, outputs of `capacity` rows); 0: out of range. */
long long global_map_bytes(int S, int MK, int n, int capacity);
/* One thread per stream.  mode 0, a streaming call: a stream with active[s] == 0 (active NULL: none) keeps every word; one
 * with restart[s] != 0 (NULL: none) gets count = built = total = 0 and dirty = 1 first; then frame_id[s] >= 0 with frame_id[s]
 * % stride == 0 is banked at slot = count (bank_frame = frame_id[s], bank_len = lengths[s] clamped to [0, n], NULL: n; count +
 * 1), or sets *overflow where count == MK.  mode 1, a rebuild: every stream gets built = total = 0 and dirty = 1.  todo =
 * min(count - built, E). */
void global_map_begin_kernel_wrapper(int S, int MK, int n, int stride, int E, int mode, const int *active,
                                     const int *restart, const int *frame_id, const int *lengths, int *state,
                                     int *bank_frame, int *bank_len, int *overflow);
/* bank_cloud[s][slot] = cloud[s] (S,n,3), all n rows, for the streams with slot >= 0. */
void global_map_push_kernel_wrapper(int S, int MK, int n, const float *cloud, const int *state, float *bank_cloud);
/* keys and rows all ones for the streams with run and dirty. */
void global_map_clear_kernel_wrapper(int S, int MK, int n, const int *state, void *keys, void *rows);
/* Grid (ceil(n/256), E, S): rows of keyframe built + blockIdx.y < built + todo enter the table; slots = the slot, -1 for a
 * row that is no candidate. */
void global_map_insert_kernel_wrapper(int S, int MK, int n, int E, double voxel, const double *X, int frames,
                                      const float *bank_cloud, const int *bank_frame, const int *bank_len,
                                      const int *state, void *keys, void *rows, int *slots);
/* blocks[s][blockIdx.y][blockIdx.x] = the winners among the workgroup's rows. */
void global_map_count_kernel_wrapper(int S, int MK, int n, int E, const int *bank_len, const int *state, void *keys,
                                     void *rows, const int *slots, int *blocks);
/* One workgroup per stream: blocks = total + the exclusive scan of the first ceil(n/256) todo counts; total += their sum. */
void global_map_scan_kernel_wrapper(int S, int MK, int n, int *state, int *blocks);
/* Winner number r of the stream (in ascending g) goes to points[s][r] (S,capacity,3) floats and source[s][r] (S,capacity,2)
 * ints (frame id, row) where r < capacity. */
void global_map_write_kernel_wrapper(int S, int MK, int n, int E, int capacity, const double *X, int frames,
                                     const float *bank_cloud, const int *bank_frame, const int *bank_len,
                                     const int *state, void *keys, void *rows, const int *slots, const int *blocks,
                                     float *points, int *source);
/* built += todo and dirty = 0 for the streams with run. */
void global_map_end_kernel_wrapper(int S, int *state);

/* ---- 13. localisation in the global map: hashed lookup, plane fit, point-to-plane rows ---------------
 * The map of section 12 is only read: keys (S,T) 64-bit words, points (S,capacity,3) floats, source (S,capacity,2) ints and
 * the word total[s * total_stride] (M = min(max(total, 0), capacity) valid ranks); T a power of two in [2^6, 2^30].  index
 * (S,T+1) ints, slot -> rank, is the caller's (slot T: the empty marker's voxel; -1: none).  An entry is never trusted: the
 * slot found for a key h yields the candidate r = index[slot] only where 0 <= r < M, the key of points[r] (section 12's rule)
 * is valid and equals h, and, with max_source_frame (S) given, source[r][0] <= max_source_frame[s].  S <= 1024.  All pointers
 * DEVICE memory; every launcher refuses a bad argument before it launches. */

/* Bytes of the index of S streams: 4 (T + 1) each; 0: out of range. */
long long map_localize_index_bytes(int S, long long T);
/* Two launches.  Ranks [lo, M) of every stream (lo = 0 where full != 0 or refill[s] != 0 (refill (S) ints, NULL: none), else
 * max(indexed[s], 0)): the key of points[r], a
 * read-only probe from its home slot until the slot's key equals it (index[slot] = r) or an empty slot or T steps (nothing);
 * the empty marker's key goes to slot T.  Then indexed[s] = M. */
void map_index_kernel_wrapper(int S, long long T, int capacity, double voxel, const void *keys, const float *points,
                              const int *source, const int *total, int total_stride, int full, const int *refill, int *indexed,
                              int *index);
/* T[s] = init[s] (S,4,4 doubles, all 16 words) for the streams with active[s] != 0 (active NULL: all). */
void map_localize_begin_kernel_wrapper(int S, const double *init, const int *active, double *T);
/* One row of sums (section 6's layout) per 256 points of p (S,n,3): q = float32(pose[s] p) (pose (S,4,4) doubles; NULL: q = p
 * and the sensor at the origin); c = rint((double)q / voxel), usable where |q / voxel| < 2^31 on every axis; the voxels c +
 * (dx,dy,dz), dz outermost, dx innermost, each in [-radius, radius], radius 1 or 2, skipping coordinates of magnitude >=
 * 2^31; the candidates in that order; the nearest by float32 sqrtf((dx dx + dy dy) + dz dz), strict <; the plane from the
 * mean and then the covariance of all candidates in fp64; no pair where the query is unusable, count < min_neighbours,
 * !(d <= max_dist), or the rank test fails.  0 <= max_dist <= radius * voxel.  rank, count, dist (S,n) and normal (S,n,3), or
 * all NULL: the nearest candidate's rank (-1: none), the number of candidates, d (+Inf: none) and the plane's unit normal
 * (0: no plane was fitted).  A stream with active[s] == 0 (NULL: none) gets zero rows and nothing else is written. */
void map_localize_accumulate_kernel_wrapper(int S, int n, long long T, int capacity, double voxel, int radius,
                                            const void *keys, const float *points, const int *source, const int *total,
                                            int total_stride, const int *index, const float *p, const double *pose,
                                            const int *max_source_frame, double sigma, float max_dist, int min_neighbours,
                                            double *partial, int *rank, int *count, float *dist, float *normal,
                                            const int *active);

#ifdef __cplusplus
}
#endif
#endif /* PWCLO_OPS_H */
