// common.h -- context, error handling and per-kernel hipEvent timing shared by all paths of libcubeslam_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"

struct cs_timing_rec {
    double total_ms = 0;
    long count = 0;
};

int cs_host_threads(); // ctx.hip
struct cs_ctx;
int cs_comm_allreduce_sum_f64(cs_ctx *ctx, double *device_buf, long n); // ctx.hip: ncclAllReduce(sum, double) in place on the context's stream
void cs_omp_prepare();
// orb.hip: device-resident results of the last cs_orb_run for one frame (keypoints in mvKeys order, 4 x u64 descriptors), for
// consumers inside the library that must not round-trip through the host (match.hip)
struct cs_orb;
int cs_orb_device_frame(const cs_orb *e, int frame, const cs_keypoint **d_kps, const unsigned long long **d_desc, int *n);  // ctx.hip: call before an OpenMP region of a host stage

// orb.hip: the resident pyramid (mvImagePyramid, ORBextractor.h:85) and the scale tables of an extractor, for stereo.hip.  Level l of frame f is
// d_pyr + f * frame_stride + off[l], w[l] x h[l] bytes, rows w[l] apart.
constexpr int CS_ORB_MAX_LEVELS = 16;
struct cs_orb_pyramid_view {
    const uint8_t *d_pyr;
    long frame_stride;
    int nlevels, n_frames, W, H;
    long off[CS_ORB_MAX_LEVELS];
    int w[CS_ORB_MAX_LEVELS], h[CS_ORB_MAX_LEVELS];
    float scale[CS_ORB_MAX_LEVELS], inv_scale[CS_ORB_MAX_LEVELS]; // mvScaleFactor / mvInvScaleFactor
    float scale_factor;
};
int cs_orb_device_pyramid(const cs_orb *e, cs_orb_pyramid_view *out);

// match.hip: the grid of the frame a matcher searches (Frame::AssignFeaturesToGrid over mvKeysUn), for klt.hip's closest-feature walk.  d_cell_recs holds KltCellRec
// records (klt_math.h) in cell order.
struct cs_matcher;
struct cs_matcher_grid_view { int N; float minX, minY, wInv, hInv; const int *d_cell_start; const void *d_cell_recs; };
int cs_matcher_device_grid(const cs_matcher *m, cs_matcher_grid_view *out);

struct cs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool timing = false;
    int host_threads = 1; // CPUs this process may really use (affinity mask and cgroup CPU quota), see cs_host_threads()
    void *comm = nullptr;  // RCCL communicator of this rank (cs_comm_init, ctx.hip); collectives run on `stream`
    int comm_rank = 0, comm_world = 1;
    std::map<std::string, cs_timing_rec> timings;
    struct pending_ev { std::string name; hipEvent_t a, b; };
    std::vector<pending_ev> pending;
    std::vector<hipEvent_t> pool;
    // Device blocks kept for reuse while `pooling` is on (the per-frame drop-in calls build and drop a whole batch per call: ~35 hipMalloc / hipFree,
    // which the driver serialises across threads).  Sizes are rounded up to a quarter-octave bucket; at most POOL_CAP bytes stay cached.
    bool pooling = false;
    std::map<void *, size_t> pool_live;
    std::multimap<size_t, void *> pool_free;
    size_t pool_cached = 0;
    static size_t pool_bucket(size_t n) {
        size_t b = 4096;
        while (b < n) b <<= 1;                       // next power of two
        const size_t q = b >> 3;                     // ... refined downwards in eighths of it
        while (b - q >= n && b - q > (b >> 1)) b -= q;
        return b;
    }
    hipError_t pool_alloc(void **p, size_t n) {
        const size_t b = pool_bucket(n);
        auto it = pool_free.find(b);
        if (it != pool_free.end()) { *p = it->second; pool_free.erase(it); pool_cached -= b; pool_live[*p] = b; return hipSuccess; }
        hipError_t e = hipMalloc(p, b);
        if (e != hipSuccess && !pool_free.empty()) { (void)hipGetLastError(); pool_drop(); e = hipMalloc(p, b); } // out of memory with blocks of other sizes cached: give those back and ask again
        if (e == hipSuccess) pool_live[*p] = b;
        return e;
    }
    void pool_release(void *p) { // a block of the pool goes back to it (or to the driver when the cache is full); anything else is freed
        auto it = pool_live.find(p);
        if (it == pool_live.end()) { hipFree(p); return; }
        const size_t b = it->second;
        pool_live.erase(it);
        constexpr size_t POOL_CAP = (size_t)1 << 30;
        if (pool_cached + b > POOL_CAP) { hipFree(p); return; }
        pool_free.emplace(b, p); pool_cached += b;
    }
    void pool_drop() { for (auto &kv : pool_free) hipFree(kv.second); pool_free.clear(); pool_cached = 0; }

    hipEvent_t get_event() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e; hipEventCreate(&e); return e;
    }
    void begin(const char *name) { begin_on(name, stream); }
    void end() { end_on(stream); }
    // the same pair around a launch on another stream of this context: both events belong to the stream the launch is on (bg_launch)
    void begin_on(const char *name, hipStream_t s) {
        if (!timing) return;
        pending_ev p; p.name = name; p.a = get_event(); p.b = get_event();
        hipEventRecord(p.a, s);
        pending.push_back(p);
    }
    void end_on(hipStream_t s) {
        if (!timing) return;
        hipEventRecord(pending.back().b, s);
    }
    // A second, lowest-priority stream of this context for ONE kind of launch: a kernel that holds its wave slots for ~100 ms and paces itself (the LSD region
    // walk), with the few small launches and copies that hand its counts to the host queued behind it.  Everything else of the context runs at the context's own
    // priority beside it.  bg_begin orders it behind `stream` with an event (a wait of the few short kernels in front of the walk, in the background stream's own
    // queue); the way back is a wait of the HOST, bg_end: a device-side wait for the walk would sit at the head of `stream`'s hardware queue for the walk's ~100 ms,
    // and where the runtime has put a second stream onto that queue (more streams of a priority than GPU_MAX_HW_QUEUES) it would hold up that stream's kernels too.
    hipStream_t bg_stream = nullptr; hipEvent_t bg_in = nullptr;
    // a second stream, at DEFAULT priority, for a branch of a launch chain that reads nothing of the other branch (cs_cuboid_batch_run); created on first use.  At the
    // context's own priority (hipStreamGetPriority of `stream`) config 4's batch measured 64.5 k frames/s against 65.3 k, three alternating runs each, so it stays as it is.
    hipStream_t aux_stream = nullptr;
    hipError_t aux_get(hipStream_t *s) {
        const hipError_t e = aux_stream ? hipSuccess : hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking);
        *s = aux_stream;
        return e;
    }
    hipError_t drain() { // every stream that work on a handle's blocks may run on (bg_stream: nothing joins it into `stream` on the device, and a call that failed between bg_begin and bg_end has left it running)
        hipError_t e = hipStreamSynchronize(stream);
        if (e == hipSuccess && aux_stream) e = hipStreamSynchronize(aux_stream);
        return e == hipSuccess && bg_stream ? hipStreamSynchronize(bg_stream) : e;
    }
    hipError_t bg_begin() { // work queued on `stream` so far precedes what is queued on bg_stream from here on
        hipError_t e = hipSuccess;
        if (!bg_stream) {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) e = hipStreamCreateWithPriority(&bg_stream, hipStreamNonBlocking, lo);
            else e = hipStreamCreateWithFlags(&bg_stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&bg_in, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        e = hipEventRecord(bg_in, stream);
        return e == hipSuccess ? hipStreamWaitEvent(bg_stream, bg_in, 0) : e;
    }
    // ... and the calling thread waits until bg_stream has run everything queued on it.  Only then may the caller launch, on any stream, what reads the results of
    // the background launches or reuses their memory: nothing on the device orders `stream` behind bg_stream.
    hipError_t bg_end() { return hipStreamSynchronize(bg_stream); }
    void flush() {
        if (pending.empty()) return;
        drain(); // (the events of a background launch are bg_stream's)
        for (auto &p : pending) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { auto &r = timings[p.name]; r.total_ms += ms; r.count++; }
            pool.push_back(p.a); pool.push_back(p.b);
        }
        pending.clear();
    }
};

#define CS_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            char b__[512];                                                                        \
            snprintf(b__, sizeof b__, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
            (ctx)->err = b__;                                                                     \
            return CS_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

// Launch helper: named, timed when ctx->timing is on.  The events of a timed launch are recorded on ctx->stream: CS_LAUNCH_ON with another stream only while timing is off.
#define CS_LAUNCH_ON(ctx, on_stream, name, kernel, grid, block, shmem, ...)           \
    do {                                                                              \
        (ctx)->begin(name);                                                           \
        hipLaunchKernelGGL(kernel, grid, block, shmem, on_stream, __VA_ARGS__);       \
        (ctx)->end();                                                                 \
    } while (0)
#define CS_LAUNCH(ctx, name, kernel, grid, block, shmem, ...) CS_LAUNCH_ON(ctx, (ctx)->stream, name, kernel, grid, block, shmem, __VA_ARGS__)
// ... and on the context's background stream, between bg_begin and bg_end: timed or not, with its events on that stream
#define CS_LAUNCH_BG(ctx, name, kernel, grid, block, shmem, ...)                            \
    do {                                                                                    \
        (ctx)->begin_on(name, (ctx)->bg_stream);                                            \
        hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->bg_stream, __VA_ARGS__);      \
        (ctx)->end_on((ctx)->bg_stream);                                                    \
    } while (0)

// The rule for device blocks: a block is obtained only through cs_dalloc (or a cs_owner, which calls it) and returned only through cs_dfree (or the owner).
// cs_dalloc may hand out a block of the context's pool, which only cs_dfree knows how to give back; no file but this one and ctx.hip calls hipMalloc / hipFree
// for a device block (the ring of frontend.hip excepted, see there).
template <class T> static inline int cs_dalloc(cs_ctx *ctx, T **p, size_t n) {
    if (n == 0) n = 1;
    if (ctx->pooling) CS_HIP(ctx, ctx->pool_alloc((void **)p, n * sizeof(T)));
    else CS_HIP(ctx, hipMalloc((void **)p, n * sizeof(T)));
    return CS_OK;
}
static inline void cs_dfree(cs_ctx *ctx, void *p) { if (!p) return; if (ctx) ctx->pool_release(p); else hipFree(p); } // (pool_release frees what the pool does not know)
template <class T> static inline int cs_h2d(cs_ctx *ctx, T *d, const T *h, size_t n) {
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return CS_OK;
}
template <class T> static inline int cs_d2h(cs_ctx *ctx, T *h, const T *d, size_t n) {
    if (n == 0) return CS_OK;
    CS_HIP(ctx, hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return CS_OK;
}
#define CS_TRY(call) do { const int r__ = (call); if (r__ != CS_OK) return r__; } while (0)
// CSR offsets of n ranges as the entry points take them: they start at 0 and do not decrease; rows may be NULL only when there is no row
static inline bool cs_offsets_ok(const int *off, int n, const void *rows) {
    if (!off || off[0] != 0) return false;
    for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return off[n] == 0 || rows;
}

// The device blocks of a handle or of one call.  Every block is allocated through alloc() and released by free_all(): there is no second list to keep.  The stream that
// may still use a block must have drained before free_all() -- the destroy functions synchronise first, a call's scratch goes through cs_scratch.
struct cs_owner {
    std::vector<void *> blocks;
    template <class T> int alloc(cs_ctx *ctx, T **p, size_t n) {
        CS_TRY(cs_dalloc(ctx, p, n));
        blocks.push_back(*p);
        return CS_OK;
    }
    template <class T> int upload(cs_ctx *ctx, T **p, const T *h, size_t n) { // alloc() + an asynchronous copy of n elements from the host
        CS_TRY(alloc(ctx, p, n));
        return cs_h2d(ctx, *p, h, n);
    }
    void free_one(cs_ctx *ctx, void *p) { blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end()); cs_dfree(ctx, p); }
    void free_all(cs_ctx *ctx) { for (void *p : blocks) cs_dfree(ctx, p); blocks.clear(); }
    void adopt(cs_owner &o) { blocks.insert(blocks.end(), o.blocks.begin(), o.blocks.end()); o.blocks.clear(); } // o's blocks are this owner's from here on
};
// the scratch of one call: released on every way out of the call, after the stream has drained (drain() is the call's own wait for its results;
// a call that keeps a wait of its own, for the error text it reports, sets `drained` behind it)
struct cs_scratch : cs_owner {
    cs_ctx *ctx; bool drained = false;
    explicit cs_scratch(cs_ctx *c) : ctx(c) {}
    int drain() { drained = true; CS_HIP(ctx, hipStreamSynchronize(ctx->stream)); return CS_OK; }
    ~cs_scratch() { if (!drained) hipStreamSynchronize(ctx->stream); free_all(ctx); }
};
// a device array that grows to what a call needs (each array has its OWN capacity: ADVICE r5 -- one cap shared by arrays of different needs let the smaller one overflow)
template <class T> struct cs_dbuf {
    T *p = nullptr; size_t cap = 0;
    int grow(cs_ctx *ctx, cs_owner &own, size_t need) {
        if (p && need <= cap) return CS_OK;
        if (p) { own.free_one(ctx, p); p = nullptr; cap = 0; }
        const size_t c = need + need / 4 + 64;
        CS_TRY(own.alloc(ctx, &p, c));
        cap = c;
        return CS_OK;
    }
};
// A host buffer in pinned memory for a recurring hand-over: the copy engine reads / writes it directly, where a pageable std::vector costs the
// runtime a second copy through its staging buffer while the calling thread waits.  It only grows (a request beyond the capacity reallocates
// and does not keep the contents); the owner calls release().  A copy into or out of it is asynchronous: synchronise before the host reads it
// or writes it again.
template <class T> struct cs_pinned {
    T *p = nullptr;
    size_t cap = 0;
    int reserve(cs_ctx *ctx, size_t n) {
        if (n <= cap) return CS_OK;
        release();
        const size_t c = n + n / 4 + 256;
        void *q = nullptr;
        CS_HIP(ctx, hipHostMalloc(&q, c * sizeof(T), hipHostMallocDefault));
        p = static_cast<T *>(q); cap = c;
        return CS_OK;
    }
    void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
};

// ---- device helpers -------------------------------------------------------------------------------------------
// 64-lane inclusive min-scan with DPP (row_shr 1/2/4/8 inside 16-lane rows, then row_bcast:15 / row_bcast:31).
__device__ __forceinline__ int wave_incl_min_scan(int x) {
    const int id = 0x7fffffff;
    int t;
    t = __builtin_amdgcn_update_dpp(id, x, 0x111, 0xf, 0xf, false); x = min(x, t); // row_shr:1
    t = __builtin_amdgcn_update_dpp(id, x, 0x112, 0xf, 0xf, false); x = min(x, t); // row_shr:2
    t = __builtin_amdgcn_update_dpp(id, x, 0x114, 0xf, 0xf, false); x = min(x, t); // row_shr:4
    t = __builtin_amdgcn_update_dpp(id, x, 0x118, 0xf, 0xf, false); x = min(x, t); // row_shr:8
    t = __builtin_amdgcn_update_dpp(id, x, 0x142, 0xa, 0xf, false); x = min(x, t); // row_bcast:15 -> rows 1,3
    t = __builtin_amdgcn_update_dpp(id, x, 0x143, 0xc, 0xf, false); x = min(x, t); // row_bcast:31 -> rows 2,3
    return x;
}
__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// The set bits of mask (a __ballot) below `lane`: the position of a flagged lane among the flagged lanes of its wave, in lane order -- the order of a push_back loop over the lanes.
__device__ __forceinline__ int wave_rank(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }
// Inclusive add-scan by a __shfl_up tree over groups of WIDTH consecutive lanes; lane: the lane's index in its group.  (The group's sum is in its last lane.)
template <int WIDTH = 64> __device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < WIDTH; off <<= 1) { const int t = __shfl_up(v, off, WIDTH); if (lane >= off) v += t; }
    return v;
}
// The two workgroup-wide forms below, for a workgroup of WAVES full waves.  Every thread of the workgroup calls them (from uniform control flow); a call costs two
// barriers; s_w holds WAVES ints and is free again behind the call.  Nothing orders what the caller stores at the returned positions: a read of it by another
// thread needs a barrier of the caller's.
// wave_sum, as lane 63 of each wave holds it -> the sum over the waves in front of the caller's; *total: over all waves
template <int WAVES> __device__ __forceinline__ int block_waves_before(int wave_sum, int *s_w, int *total) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = wave_sum;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { const int c = s_w[w]; before += w < wave ? c : 0; all += c; }
    __syncthreads();
    *total = all;
    return before;
}
// exclusive prefix of v over the threads of the workgroup, in thread order; *total: the workgroup's sum
template <int WAVES> __device__ __forceinline__ int block_excl_scan(int v, int *s_w, int *total) {
    const int inc = wave_incl_scan(v, threadIdx.x & 63);
    return block_waves_before<WAVES>(inc, s_w, total) + inc - v;
}
// The position of a flagged thread among the flagged threads of the workgroup, in thread order (where a thread stands for element base + threadIdx.x, the order of the
// reference's push_back loop over the elements); *total: their number.  The return value means something only where flag is set.
template <int WAVES> __device__ __forceinline__ int block_rank(bool flag, int *s_w, int *total) {
    const unsigned long long b = __ballot(flag);
    return block_waves_before<WAVES>(__popcll(b), s_w, total) + wave_rank(b, threadIdx.x & 63);
}
// Hamming distance of two 256-bit descriptors, four u64 words each (ORBmatcher::DescriptorDistance)
__device__ __forceinline__ int hamming256(const unsigned long long *a, unsigned long long b0, unsigned long long b1, unsigned long long b2, unsigned long long b3) {
    return __popcll(a[0] ^ b0) + __popcll(a[1] ^ b1) + __popcll(a[2] ^ b2) + __popcll(a[3] ^ b3);
}

// The sums of a 256-thread workgroup, in one fixed order of additions (the optimisers' results depend on it): the lanes of a wave by a shuffle tree 32 .. 1,
// then the four wave results as (w0 + w1) + (w2 + w3).  s_red holds 4 x N doubles.
template <int N> __device__ __forceinline__ void block_reduce_waves(double (&v)[N], double *s_red) { // -> s_red[wave * N + k], readable behind the call
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if (lane == 0) for (int k = 0; k < N; k++) s_red[wave * N + k] = v[k];
    __syncthreads();
}
template <int N> __device__ __forceinline__ double block_reduce_sum(const double *s_red, int k) { return (s_red[k] + s_red[N + k]) + (s_red[2 * N + k] + s_red[3 * N + k]); }
// N values per thread -> s_out[0 .. N), which every thread may read behind the call
template <int N> __device__ __forceinline__ void block_reduce(double (&v)[N], double *s_red, double *s_out) {
    block_reduce_waves(v, s_red);
    if (threadIdx.x < N) s_out[threadIdx.x] = block_reduce_sum<N>(s_red, threadIdx.x);
    __syncthreads();
}
// one value per thread -> partials[bid]: the workgroup's share of a sum the host (or a later kernel) finishes over the small partial array
__device__ inline void block_sum_store(double v, double *partials, int bid) {
    __shared__ double s[4];
    double w[1] = {v};
    block_reduce_waves(w, s);
    if (threadIdx.x == 0) partials[bid] = block_reduce_sum<1>(s, 0);
}

// Four neighbouring pixels of a u8 row with one load.  gfx950 runs global memory in unaligned-access mode (a dword load may start at
// any byte; tools/ubench/unaligned_load.hip checks it on the device), and one dword gather costs the texture-address unit a quarter
// of four byte gathers.
typedef uint32_t __attribute__((aligned(1))) cs_u32_unaligned;
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) { return *reinterpret_cast<const cs_u32_unaligned *>(p); }

// four consecutive bytes of the 12-byte window w0 w1 w2 starting at byte START (0..8), as one dword
template <int START> __device__ __forceinline__ uint32_t win4(uint32_t w0, uint32_t w1, uint32_t w2) {
    if (START == 0) return w0;
    if (START < 4) return __builtin_amdgcn_alignbyte(w1, w0, START);
    if (START == 4) return w1;
    if (START < 8) return __builtin_amdgcn_alignbyte(w2, w1, START - 4);
    return w2;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the global-memory counter (s_waitcnt vmcnt(0)), so
// in a loop that stores a result row / column to global memory and prefetches the next one, every barrier would wait for those
// round trips (measured: 5.4 us per column in ba_band_chol, 3.5 us per row in orb_blur).  Only valid where no thread reads,
// through a cached path, global data another thread of the workgroup wrote before the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
