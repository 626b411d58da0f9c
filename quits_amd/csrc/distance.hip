// distance.hip -- the random information-set estimate of the distance (qd_isd_*; the definition and its numpy mirror are quits_amd/distance.py).
// One trial = one random column order of H and one GF(2) elimination along it; one workgroup runs one trial at a time, in a grid that loops
// over the trials of a call.  Nothing in a trial depends on the grid: rec[t] is a function of (model, seed, t).
//
// A trial.  (1) keys: Philox4x32-10, counter (t lo, t hi, j >> 2, 4), word j & 3; the 64-bit words key << 32 | j are sorted in LDS (bitonic, padded
// to a power of two with all-ones words) and their low halves written to the workgroup's slice of device memory: the order.  (2) The same LDS
// then holds the row transform BY DETECTOR: row d = the W = ceil(m / 32) words of column d of R, then two words of mask.  For any column h of H
// the XOR of the rows of its support is (R h, mask of the pivots R h names); R h lies inside the pivot rows iff h is dependent, its popcount + 1
// is then the weight of the kernel vector h closes and its mask words XOR fault_obs the observables that vector flips.  (3) The order is walked
// in blocks of B = threads / G columns, G lanes to a column: the block's columns are reduced in parallel into LDS; the first independent one
// (LDS atomicMin of the block index) becomes a pivot on its lowest free row r, everything before it is a candidate; the pivot's reduced vector
// u (bit r cleared, its mask words = the pivot's whole mask) is XORed into every row of the transform and every later column of the block that
// has bit r -- that is the row operation R <- (I + u e_r^T) R seen by columns.  Two barriers a pivot; a block without an independent column --
// every block once the rank is complete -- is one parallel pass.  Candidates with a non-zero mask go to an LDS histogram and a running minimum
// per lane, folded with one 64-bit LDS atomicMin per group at the end of the trial.
//
// Why the masks ride along.  Write M for the two mask words as a 64 x m matrix: M = Lambda R, Lambda holding fault_obs of the pivot that owns row r in
// column r.  A new pivot p on row r with v = R h_p turns R into E R, E = I + (v + e_r) e_r^T, and Lambda into Lambda + obs(p) e_r^T; since e_r^T E = e_r^T
// and Lambda e_r was 0, M becomes M + (M h_p + obs(p)) (row r of R).  So column d of [R; M] changes by (v + e_r, M h_p + obs(p)) iff R[r][d] = 1: one
// vector u for all m + 64 bits, and M h_p + obs(p) is what the block already holds in the mask words of column p.
//
// Bounds.  qd_isd_create checks every detector index of col_rows against ndet and col_ptr against nnz, so LDS row indices stay below m; the
// order holds low halves of sorted words whose low halves are 0 .. n - 1 (padding words sort last and are not read).
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#include <memory>

#define QD_ISD_MAX_THREADS 1024
#define QD_ISD_MAX_SORT 16384               // words of 8 bytes sorted in LDS: 128 KiB
#define QD_ISD_HEAD 72                      // header words of the LDS image: record (2), first-independent slots (2), pivot row (1), pad, histogram (64)
#define QD_ISD_STREAM 4u                    // last Philox counter word (qd_sample_dem 0, qd_sample_circuit 1, strata 2, Relay-BP 3)
#define QD_ISD_NONE 0xFFFFFFFFFFFFFFFFull

typedef unsigned long long u64;

struct IsdDev {
    const uint32_t *col_ptr;        // [n + 1]
    const uint32_t *col_rows;       // [nnz] detectors of every fault, all < m
    const u64 *fault_obs;           // [n]
    uint32_t *order_ws;             // [grid_max][n] the order of the trial a workgroup runs
    u64 *hist;                      // [QD_ISD_HIST]
    int32_t *rank;                  // [1] pivots of the last trial run (the same in every trial)
    int m, n, W, S, G, B, P, head;  // S: row stride in words (W + 2 made odd); G lanes a column, B columns a block; P: sorted words; head: header + pivot-row mask words
};

struct qd_isd {
    IsdDev d;
    DevAllocs mem;
    int device = 0, threads = 0, lds = 0, grid_max = 0;
    size_t ws_bytes = 0;
    hipStream_t last = nullptr;
    ~qd_isd() { mem.release(); }
};

__device__ __forceinline__ uint32_t isd_group_or(uint32_t x, int G)
{
    for (int o = G >> 1; o > 0; o >>= 1) x |= (uint32_t)__shfl_xor((int)x, o, 64);
    return x;
}
__device__ __forceinline__ uint32_t isd_group_add(uint32_t x, int G)
{
    for (int o = G >> 1; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, 64);
    return x;
}
__device__ __forceinline__ uint32_t isd_group_min(uint32_t x, int G)
{
    for (int o = G >> 1; o > 0; o >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}

__global__ void __launch_bounds__(QD_ISD_MAX_THREADS) qd_isd_kernel(IsdDev a, u64 seed, u64 trial0, u64 ntrials, u64 *__restrict__ records)
{
    extern __shared__ __align__(16) uint32_t isd_lds[];
    u64 *rec = reinterpret_cast<u64 *>(isd_lds);
    uint32_t *first = isd_lds + 2;              // two slots, used by alternate pivot steps
    uint32_t *rsel = isd_lds + 4;
    uint32_t *hist = isd_lds + 8;
    uint32_t *piv = isd_lds + QD_ISD_HEAD;      // [W] rows that hold a pivot
    uint32_t *state = isd_lds + a.head;         // [m][S]; before that, the sort's P words of 8 bytes (head is even)
    u64 *keys = reinterpret_cast<u64 *>(state);
    uint32_t *blk = state + (size_t)a.m * a.S;  // [B][S]
    const int tid = threadIdx.x, T = blockDim.x;
    const int m = a.m, n = a.n, W = a.W, S = a.S, G = a.G, B = a.B, KW = a.W + 2;
    const int g = tid / G, lane = tid % G;
    uint32_t *order = a.order_ws + (size_t)blockIdx.x * n;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);

    for (u64 t = blockIdx.x; t < ntrials; t += gridDim.x) {
        const u64 trial = trial0 + t;
        __syncthreads();                                                    // the previous trial has left LDS
        // ---- the order
        for (int c = tid; 4 * c < a.P; c += T) {
            uint32_t r[4] = {0, 0, 0, 0};
            if (4 * c < n) qd_philox4x32_10((uint32_t)trial, (uint32_t)(trial >> 32), (uint32_t)c, QD_ISD_STREAM, k0, k1, r);
            keys[4 * c + 0] = 4 * c + 0 < n ? ((u64)r[0] << 32) | (uint32_t)(4 * c + 0) : QD_ISD_NONE;
            keys[4 * c + 1] = 4 * c + 1 < n ? ((u64)r[1] << 32) | (uint32_t)(4 * c + 1) : QD_ISD_NONE;
            keys[4 * c + 2] = 4 * c + 2 < n ? ((u64)r[2] << 32) | (uint32_t)(4 * c + 2) : QD_ISD_NONE;
            keys[4 * c + 3] = 4 * c + 3 < n ? ((u64)r[3] << 32) | (uint32_t)(4 * c + 3) : QD_ISD_NONE;
        }
        for (int k = 2; k <= a.P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int i = tid; i < (a.P >> 1); i += T) {
                    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                    const u64 x = keys[lo], y = keys[hi];
                    if ((x > y) == ((lo & k) == 0)) {
                        keys[lo] = y;
                        keys[hi] = x;
                    }
                }
            }
        __syncthreads();
        for (int i = tid; i < n; i += T) order[i] = (uint32_t)keys[i];
        __syncthreads();                                                    // the order is in device memory, LDS is free again
        // ---- the transform: R = I, no masks, no pivots
        for (int i = tid; i < m * S; i += T) state[i] = 0;
        if (tid < 64) hist[tid] = 0;
        if (tid == 0) {
            *rec = QD_ISD_NONE;
            first[0] = first[1] = (uint32_t)B;
        }
        for (int k = tid; k < W; k += T) piv[k] = 0;
        __syncthreads();
        for (int d = tid; d < m; d += T) state[(size_t)d * S + (d >> 5)] = 1u << (d & 31);
        u64 best = QD_ISD_NONE;
        int npiv = 0;
        uint32_t it = 0;
        // ---- the walk
        for (int base = 0; base < n; base += B) {
            __syncthreads();                                                // the transform is whole
            const bool have = base + g < n;
            uint32_t j = 0;
            if (have) {
                j = order[base + g];
                j = j < (uint32_t)n ? j : 0;
                const uint32_t p0 = a.col_ptr[j], p1 = a.col_ptr[j + 1];
                const u64 fo = a.fault_obs[j];
                for (int k = lane; k < KW; k += G) {
                    uint32_t x = k == W ? (uint32_t)fo : k == W + 1 ? (uint32_t)(fo >> 32) : 0u;
                    for (uint32_t p = p0; p < p1; ++p) x ^= state[(size_t)a.col_rows[p] * S + k];
                    blk[g * S + k] = x;
                }
            }
            int cur = 0;                                                    // block columns below cur are settled
            for (;;) {
                uint32_t indep = 0;
                if (have && g >= cur)
                    for (int k = lane; k < W; k += G) indep |= blk[g * S + k] & ~piv[k];
                indep = isd_group_or(indep, G);
                if (indep && lane == 0) atomicMin(first + (it & 1), (uint32_t)g);
                __syncthreads();
                const int f = (int)first[it & 1];
                if (have && g >= cur && g < f) {                             // a candidate
                    uint32_t w = 0;
                    for (int k = lane; k < W; k += G) w += __popc(blk[g * S + k]);
                    w = isd_group_add(w, G) + 1;
                    if (lane == 0 && (blk[g * S + W] | blk[g * S + W + 1])) {
                        atomicAdd(hist + (w < 63 ? w : 63), 1u);
                        const u64 v = ((u64)w << 32) | j;
                        best = v < best ? v : best;
                    }
                }
                if (f >= B) break;
                if (g == f) {                                               // the pivot: its lowest free row
                    uint32_t r = 0xFFFFFFFFu;
                    for (int k = lane; k < W; k += G) {
                        const uint32_t x = blk[g * S + k] & ~piv[k];
                        if (x && r == 0xFFFFFFFFu) r = 32u * k + (uint32_t)__ffs(x) - 1u;
                    }
                    r = isd_group_min(r, G);
                    if (lane == 0) {
                        *rsel = r;
                        blk[g * S + (r >> 5)] &= ~(1u << (r & 31));
                        piv[r >> 5] |= 1u << (r & 31);
                    }
                }
                if (tid == 0) first[(it + 1) & 1] = (uint32_t)B;
                __syncthreads();
                const uint32_t r = *rsel, rw = r >> 5, rb = 1u << (r & 31);
                const uint32_t *u = blk + f * S;
                for (int d = tid; d < m; d += T)
                    if (state[(size_t)d * S + rw] & rb)
                        for (int k = 0; k < KW; ++k) state[(size_t)d * S + k] ^= u[k];
                if (have && g > f && (blk[g * S + rw] & rb))
                    for (int k = lane; k < KW; k += G) blk[g * S + k] ^= u[k];
                cur = f + 1;
                npiv += 1;
                it += 1;
            }
        }
        if (lane == 0 && best != QD_ISD_NONE) atomicMin(rec, best);
        __syncthreads();
        if (tid < 64 && hist[tid]) atomicAdd(a.hist + tid, (u64)hist[tid]);
        if (tid == 0) {
            records[t] = *rec;
            *a.rank = npiv;
        }
    }
}

static int isd_pow2_at_least(int x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

extern "C" int qd_isd_create(int32_t ndet, int32_t n, const int64_t *col_ptr, const int32_t *col_rows, const uint64_t *fault_obs, int32_t device,
                             qd_isd **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (ndet < 1 || ndet > 65535 || n < 1) return qd_fail(QD_EINVAL, "%d detectors and %d faults: 1 .. 65535 detectors, at least one fault", ndet, n);
    if (!col_ptr || !fault_obs) return qd_fail(QD_EINVAL, "null argument");
    if (col_ptr[0] != 0) return qd_fail(QD_EINVAL, "col_ptr[0] must be 0");
    std::vector<uint32_t> cp((size_t)n + 1);
    for (int j = 0; j < n; ++j) {
        if (col_ptr[j + 1] < col_ptr[j] || col_ptr[j + 1] > (int64_t)0x7FFFFFFF) return qd_fail(QD_EINVAL, "col_ptr is not a CSC pointer array at column %d", j);
        cp[j + 1] = (uint32_t)col_ptr[j + 1];
    }
    const size_t nnz = cp[n];
    if (nnz && !col_rows) return qd_fail(QD_EINVAL, "null argument");
    std::vector<uint32_t> cr(nnz);
    for (size_t x = 0; x < nnz; ++x) {
        if (col_rows[x] < 0 || col_rows[x] >= ndet) return qd_fail(QD_EINVAL, "col_rows[%zu] = %d is no detector", x, col_rows[x]);
        cr[x] = (uint32_t)col_rows[x];
    }
    std::unique_ptr<qd_isd> s(new qd_isd());
    IsdDev &d = s->d;
    d.m = ndet; d.n = n;
    d.W = (ndet + 31) / 32;
    d.S = (d.W + 2) | 1;                                                    // an odd stride: rows a lane apart fall on different banks
    d.G = std::min(16, std::max(4, isd_pow2_at_least(d.W + 2)));
    s->threads = ndet <= 64 ? 64 : ndet <= 256 ? 256 : QD_ISD_MAX_THREADS;  // a small model runs one wavefront a trial, many trials a CU
    d.B = s->threads / d.G;
    d.P = std::max(4, isd_pow2_at_least(n));
    d.head = (QD_ISD_HEAD + d.W + 1) & ~1;
    const size_t sort_bytes = 4 * (size_t)d.head + 8 * (size_t)d.P;
    const size_t form_bytes = 4 * ((size_t)d.head + ((size_t)ndet + d.B) * d.S);
    if (form_bytes > QD_LDS_BYTES)
        return qd_fail(QD_ECAPACITY, "the row transform of %d detectors takes %zu bytes of LDS, a CU holds %d (a device-memory form is not implemented)", ndet,
                       form_bytes, QD_LDS_BYTES);
    if (n > QD_ISD_MAX_SORT || sort_bytes > QD_LDS_BYTES)
        return qd_fail(QD_ECAPACITY, "the order of %d faults takes %zu bytes of LDS while it is sorted, a CU holds %d (at most %d faults)", n,
                       4 * (size_t)d.head + 8 * (size_t)isd_pow2_at_least(n), QD_LDS_BYTES, QD_ISD_MAX_SORT);
    s->lds = (int)((std::max(sort_bytes, form_bytes) + 15) & ~(size_t)15);
    s->device = device;
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    // workgroups a CU holds at once: by LDS and by wavefronts (the kernel is compiled for 1024 threads: at most 128 VGPRs, 16 wavefronts a CU)
    const int per_cu = std::max(1, std::min(QD_LDS_BYTES / s->lds, QD_ISD_MAX_THREADS / s->threads));
    s->grid_max = std::max(1, prop.multiProcessorCount) * per_cu;
    s->ws_bytes = (size_t)s->grid_max * n * sizeof(uint32_t);
    // everything a run touches is allocated here: a model that does not fit fails before any launch
    if (s->mem.alloc((size_t)s->grid_max * n, &d.order_ws) != hipSuccess || s->mem.alloc((size_t)QD_ISD_HIST, &d.hist) != hipSuccess ||
        s->mem.alloc((size_t)4, &d.rank) != hipSuccess) {
        (void)hipGetLastError();
        return qd_fail(QD_EHIP, "device allocation failed: %zu bytes of column orders", s->ws_bytes);
    }
    d.col_ptr = static_cast<const uint32_t *>(s->mem.upload(cp.data(), cp.size() * sizeof(uint32_t)));
    d.col_rows = static_cast<const uint32_t *>(s->mem.upload(cr.data(), nnz * sizeof(uint32_t)));
    d.fault_obs = static_cast<const u64 *>(s->mem.upload(fault_obs, (size_t)n * sizeof(u64)));
    if (!d.col_ptr || !d.col_rows || !d.fault_obs) return qd_fail(QD_EHIP, "device allocation/upload failed");
    HIP_TRY(hipMemset(d.hist, 0, QD_ISD_HIST * sizeof(u64)));
    HIP_TRY(hipMemset(d.rank, 0xFF, sizeof(int32_t)));
    HIP_TRY(hipFuncSetAttribute((const void *)qd_isd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s->lds));
    *out = s.release();
    return QD_OK;
}

extern "C" void qd_isd_destroy(qd_isd *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}

extern "C" int qd_isd_info(qd_isd *s, int64_t *info)
{
    if (!s || !info) return qd_fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->last));
    int32_t rank = -1;
    HIP_TRY(hipMemcpy(&rank, s->d.rank, sizeof(rank), hipMemcpyDeviceToHost));
    const int64_t v[8] = {s->lds, s->threads, (int64_t)s->ws_bytes, s->grid_max, rank, s->d.B, s->d.G, s->d.P};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return QD_OK;
}

extern "C" int qd_isd_run(qd_isd *s, uint64_t seed, int64_t trial0, int64_t ntrials, uint64_t *d_records, void *stream)
{
    if (!s) return qd_fail(QD_EINVAL, "null estimator");
    if (trial0 < 0 || ntrials < 0 || (ntrials > 0 && !d_records)) return qd_fail(QD_EINVAL, "bad trial range or null records");
    if (ntrials == 0) return QD_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipFuncSetAttribute((const void *)qd_isd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, s->lds));
    s->last = st;
    const unsigned grid = (unsigned)std::min<int64_t>(ntrials, s->grid_max);
    hipLaunchKernelGGL(qd_isd_kernel, dim3(grid), dim3(s->threads), (size_t)s->lds, st, s->d, (u64)seed, (u64)trial0, (u64)ntrials,
                       reinterpret_cast<u64 *>(d_records));
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_isd_hist(qd_isd *s, uint64_t *hist)
{
    if (!s || !hist) return qd_fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->last));
    HIP_TRY(hipMemcpy(hist, s->d.hist, QD_ISD_HIST * sizeof(u64), hipMemcpyDeviceToHost));
    return QD_OK;
}

extern "C" int qd_isd_reset(qd_isd *s)
{
    if (!s) return qd_fail(QD_EINVAL, "null estimator");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->last));
    HIP_TRY(hipMemset(s->d.hist, 0, QD_ISD_HIST * sizeof(u64)));
    return QD_OK;
}
