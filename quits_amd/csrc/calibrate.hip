// calibrate.hip -- the counting pass of the prior fit (qd_bit_planes, qd_calib_*, qd_parity_counts; the definition, its numpy mirror and the fit
// itself are quits_amd/calibrate.py).  For every column of H with detectors e = (d_0 < .. < d_{s-1}), s <= 10, and every mask t = 1 .. 2^s - 1,
// c[t] = the number of shots in which the XOR of the detectors t selects is 1.  That is all the fit reads of the shots.
//
// (1) qd_bit_planes turns rows of one byte per detector into one bit plane per detector: word w of plane d holds detector d of shots
// 64 w .. 64 w + 63.  One wavefront per 64 shots, a lane per shot: __ballot of a detector's low bit IS the word.  A lane reads eight bytes of its
// own row at a time (one aligned load where the row allows it); lane i keeps the ballot of detector d0 + i, and after 64 detectors the wavefront
// stores 64 words, one per plane.  Shots at and beyond B vote 0, so the pad bits of the last word are 0.
//
// (2) qd_parity_counts.  A TASK is one wavefront's share of a column: the column's low = min(s, 6) lowest detectors span 2^low subsets, walked
// in Gray-code order -- one XOR, one popcount, one add per subset and word -- on top of a base word, the XOR of the subset h of the s - low top
// detectors; a column of weight s > 6 is 2^(s - 6) tasks, h = 0 .. 2^(s - 6) - 1 (16 at s = 10), a lighter one a single task.  The lanes
// stride over the words of the planes (coalesced); each holds 2^low 32-bit counters in registers -- the walk is unrolled, so every counter
// index is a constant -- which are summed over the wavefront once, after the word loop, and added to the 64-bit output row by the lane that
// owns the counter: out[count_ptr[j] + ((h << low) | g) - 1], g the low mask (h = g = 0 is the empty set: not stored).  Every counter has
// one owner, so there are no atomics and the sums do not depend on the grid; the tasks are independent, so there is no LDS and no barrier.
//
// Bounds.  qd_calib_create checks every detector of col_det against ndet and every column's weight against QD_CALIB_MAX_WEIGHT and builds the task
// list and count_ptr itself; qd_parity_counts checks the planes' stride against the word count.  A plane index is det * stride + w with
// det < ndet and w < nwords <= stride: inside the ndet * stride words the caller vouches for.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#include <memory>

#define QD_CALIB_THREADS 256
#define QD_CALIB_LOW 6                      // detectors walked inside a wavefront: 64 counters a lane
#define QD_CALIB_MAX_BLOCKS 16384           // both grids are bounded: a wavefront strides over its words (planes) or tasks (counts)
#define QD_CALIB_MAX_WORDS (1ll << 25)      // words per call: 2^31 shots, so that a wavefront's 32-bit sums cannot wrap

typedef unsigned long long u64;

struct CalibDev {
    const int32_t *col_ptr;         // [ncols + 1]
    const int32_t *col_det;         // [nnz] detectors of every column, ascending, all < ndet
    const int64_t *count_ptr;       // [ncols + 1] first counter of every column
    const uint32_t *tasks;          // [ntasks] column << 4 | h, heaviest first
    int ndet, ncols, ntasks;
};

struct qd_calib {
    CalibDev d;
    DevAllocs mem;
    int device = 0, max_weight = 0;
    int64_t total = 0;
    ~qd_calib() { mem.release(); }
};

__global__ void __launch_bounds__(QD_CALIB_THREADS) qd_bit_planes_kernel(const uint8_t *__restrict__ in, int64_t in_stride, int ndet, int64_t B,
                                                                         u64 *__restrict__ planes, int64_t plane_stride, int64_t nwords)
{
    const int lane = threadIdx.x & (QD_WAVE - 1), wv = threadIdx.x >> 6;
    const int64_t step = (int64_t)gridDim.x * (QD_CALIB_THREADS / QD_WAVE);
    for (int64_t w = (int64_t)blockIdx.x * (QD_CALIB_THREADS / QD_WAVE) + wv; w < nwords; w += step) {        // uniform in the wavefront
        const int64_t b = (w << 6) + lane;
        const bool live = b < B;
        const uint8_t *row = in + (live ? b : 0) * in_stride;
        const bool aligned = (reinterpret_cast<uintptr_t>(row) & 7u) == 0;
        for (int d0 = 0; d0 < ndet; d0 += QD_WAVE) {
            u64 keep = 0;
            const int dn = ndet - d0 < QD_WAVE ? ndet - d0 : QD_WAVE;
            for (int g = 0; g < dn; g += 8) {
                const int cnt = dn - g < 8 ? dn - g : 8;
                const uint8_t *p = row + d0 + g;
                u64 v = 0;
                if (live) {
                    if (cnt == 8 && aligned)                    // (d0 + g is a multiple of 8)
                        v = *reinterpret_cast<const u64 *>(p);
                    else
#pragma clang loop vectorize(disable) unroll(disable)
                        for (int i = 0; i < cnt; ++i) v |= (u64)p[i] << (8 * i);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {                   // (bytes at and beyond cnt are 0 and belong to no plane)
                    const u64 word = __ballot((v >> (8 * i)) & 1ull);
                    if (lane == g + i) keep = word;
                }
            }
            if (lane < dn) planes[(int64_t)(d0 + lane) * plane_stride + w] = keep;
        }
    }
}

// The share of one task: LOW detectors walked, `top` more selected by h into the base word.
template <int LOW>
__device__ __forceinline__ void qd_parity_task(const u64 *__restrict__ planes, int64_t stride, int64_t nwords, const int32_t *__restrict__ det, int top,
                                               int h, long long *out, int lane)
{
    constexpr int NC = 1 << LOW;
    uint32_t cnt[NC];
#pragma unroll
    for (int g = 0; g < NC; ++g) cnt[g] = 0u;
    const u64 *pl[LOW];
#pragma unroll
    for (int i = 0; i < LOW; ++i) pl[i] = planes + (int64_t)det[i] * stride;
    for (int64_t w = lane; w < nwords; w += QD_WAVE) {
        u64 x = 0;
        for (int i = 0; i < top; ++i)                           // (uniform: h and top belong to the task)
            if ((h >> i) & 1) x ^= planes[(int64_t)det[LOW + i] * stride + w];
        u64 q[LOW];
#pragma unroll
        for (int i = 0; i < LOW; ++i) q[i] = pl[i][w];
        cnt[0] += (uint32_t)__popcll(x);
#pragma unroll
        for (int k = 1; k < NC; ++k) {                          // Gray code: step k flips detector ctz(k) and lands on the mask k ^ (k >> 1)
            x ^= q[__builtin_ctz((unsigned)k)];
            cnt[k ^ (k >> 1)] += (uint32_t)__popcll(x);
        }
    }
    uint32_t mine = 0;
#pragma unroll
    for (int g = 0; g < NC; ++g) {
        const uint32_t sum = qd_wave_add(cnt[g]);
        if (lane == g) mine = sum;
    }
    const int t = (h << LOW) | lane;
    if (lane < NC && t >= 1) out[t - 1] += (long long)mine;
}

__global__ void __launch_bounds__(QD_CALIB_THREADS) qd_parity_counts_kernel(CalibDev c, const u64 *__restrict__ planes, int64_t stride, int64_t nwords,
                                                                            long long *counts)
{
    const int lane = threadIdx.x & (QD_WAVE - 1), wv = threadIdx.x >> 6;
    const int step = (int)gridDim.x * (QD_CALIB_THREADS / QD_WAVE);
    for (int k = (int)blockIdx.x * (QD_CALIB_THREADS / QD_WAVE) + wv; k < c.ntasks; k += step) {                 // uniform in the wavefront
        const uint32_t task = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.tasks[k]);
        const int j = (int)(task >> 4), h = (int)(task & 15u);
        const int32_t *det = c.col_det + c.col_ptr[j];
        const int s = __builtin_amdgcn_readfirstlane(c.col_ptr[j + 1] - c.col_ptr[j]);
        long long *out = counts + c.count_ptr[j];
        switch (s < QD_CALIB_LOW ? s : QD_CALIB_LOW) {
        case 1: qd_parity_task<1>(planes, stride, nwords, det, 0, 0, out, lane); break;
        case 2: qd_parity_task<2>(planes, stride, nwords, det, 0, 0, out, lane); break;
        case 3: qd_parity_task<3>(planes, stride, nwords, det, 0, 0, out, lane); break;
        case 4: qd_parity_task<4>(planes, stride, nwords, det, 0, 0, out, lane); break;
        case 5: qd_parity_task<5>(planes, stride, nwords, det, 0, 0, out, lane); break;
        default: qd_parity_task<QD_CALIB_LOW>(planes, stride, nwords, det, s - QD_CALIB_LOW, h, out, lane); break;
        }
    }
}

static unsigned calib_blocks(int64_t waves)
{
    const int64_t blocks = (waves + QD_CALIB_THREADS / QD_WAVE - 1) / (QD_CALIB_THREADS / QD_WAVE);
    return (unsigned)(blocks < QD_CALIB_MAX_BLOCKS ? blocks : QD_CALIB_MAX_BLOCKS);
}

extern "C" int qd_bit_planes(const uint8_t *d_in, int64_t in_stride, int32_t ndet, int64_t B, uint64_t *d_planes, int64_t plane_stride, void *stream)
{
    if (B < 0 || ndet < 0) return qd_fail(QD_EINVAL, "negative shot count or detector count");
    if (B > 64 * QD_CALIB_MAX_WORDS) return qd_fail(QD_EINVAL, "%lld shots: at most 2^31 in one call", (long long)B);
    const int64_t nwords = (B + 63) / 64;
    if (in_stride < ndet) return qd_fail(QD_EINVAL, "in_stride %lld is smaller than ndet = %d", (long long)in_stride, ndet);
    if (plane_stride < nwords) return qd_fail(QD_EINVAL, "plane_stride %lld is smaller than the %lld words of %lld shots", (long long)plane_stride,
                                              (long long)nwords, (long long)B);
    if (B == 0 || ndet == 0) return QD_OK;
    if (!d_in || !d_planes) return qd_fail(QD_EINVAL, "null detector rows or planes");
    hipLaunchKernelGGL(qd_bit_planes_kernel, dim3(calib_blocks(nwords)), dim3(QD_CALIB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), d_in, in_stride,
                       ndet, B, reinterpret_cast<u64 *>(d_planes), plane_stride, nwords);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_calib_create(int32_t ndet, int32_t ncols, const int64_t *col_ptr, const int32_t *col_det, int32_t device, qd_calib **out)
{
    if (!out) return qd_fail(QD_EINVAL, "null output handle");
    *out = nullptr;
    if (ndet < 0 || ncols < 0) return qd_fail(QD_EINVAL, "negative detector count or column count");
    if (ncols > (1 << 27)) return qd_fail(QD_EINVAL, "%d columns: at most 2^27", ncols);
    if (!col_ptr || (!col_det && ncols > 0 && col_ptr[ncols] > 0)) return qd_fail(QD_EINVAL, "null column table");
    if (col_ptr[0] != 0) return qd_fail(QD_EINVAL, "col_ptr[0] must be 0");
    std::vector<int32_t> cp((size_t)ncols + 1, 0);
    std::vector<int64_t> count_ptr((size_t)ncols + 1, 0);
    std::vector<uint32_t> tasks;
    int max_weight = 0;
    for (int low = QD_CALIB_LOW; low >= 1; --low)               // heaviest first: the long tasks start first
        for (int j = 0; j < ncols; ++j) {
            const int64_t s = col_ptr[j + 1] - col_ptr[j];
            if (low == QD_CALIB_LOW) {
                if (s < 1 || col_ptr[j + 1] > INT32_MAX) return qd_fail(QD_EINVAL, "column %d is empty or col_ptr does not ascend", j);
                if (s > QD_CALIB_MAX_WEIGHT)
                    return qd_fail(QD_ECAPACITY, "column %d has weight %lld: the counting kernel holds at most %d detectors a column", j, (long long)s,
                                   QD_CALIB_MAX_WEIGHT);
                for (int64_t x = col_ptr[j]; x < col_ptr[j + 1]; ++x) {
                    if (col_det[x] < 0 || col_det[x] >= ndet) return qd_fail(QD_EINVAL, "column %d: detector %d is outside 0 .. %d", j, col_det[x], ndet - 1);
                    if (x > col_ptr[j] && col_det[x] <= col_det[x - 1]) return qd_fail(QD_EINVAL, "column %d: its detectors do not ascend", j);
                }
                cp[(size_t)j + 1] = (int32_t)col_ptr[j + 1];
                count_ptr[(size_t)j + 1] = count_ptr[(size_t)j] + ((1ll << s) - 1);
                max_weight = std::max(max_weight, (int)s);
            }
            if ((s < QD_CALIB_LOW ? (int)s : QD_CALIB_LOW) == low)
                for (int h = 0; h < (s > QD_CALIB_LOW ? 1 << (s - QD_CALIB_LOW) : 1); ++h) tasks.push_back(((uint32_t)j << 4) | (uint32_t)h);
        }
    if (tasks.size() > (size_t)INT32_MAX) return qd_fail(QD_EINVAL, "too many tasks");
    std::unique_ptr<qd_calib> s(new qd_calib());
    s->device = device;
    s->max_weight = max_weight;
    s->total = count_ptr[(size_t)ncols];
    s->d.ndet = ndet; s->d.ncols = ncols; s->d.ntasks = (int)tasks.size();
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    s->d.col_ptr = static_cast<const int32_t *>(s->mem.upload(cp.data(), cp.size() * sizeof(int32_t)));
    s->d.col_det = static_cast<const int32_t *>(s->mem.upload(col_det, (size_t)cp[(size_t)ncols] * sizeof(int32_t)));
    s->d.count_ptr = static_cast<const int64_t *>(s->mem.upload(count_ptr.data(), count_ptr.size() * sizeof(int64_t)));
    s->d.tasks = static_cast<const uint32_t *>(s->mem.upload(tasks.data(), tasks.size() * sizeof(uint32_t)));
    if (!s->d.col_ptr || !s->d.col_det || !s->d.count_ptr || !s->d.tasks) {
        (void)hipGetLastError();
        return qd_fail(QD_EHIP, "device allocation/upload of the column table failed");
    }
    *out = s.release();
    return QD_OK;
}

extern "C" void qd_calib_destroy(qd_calib *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    delete s;
}

extern "C" int qd_calib_info(const qd_calib *s, int64_t *info)
{
    if (!s || !info) return qd_fail(QD_EINVAL, "null argument");
    const int64_t v[4] = {s->total, s->d.ntasks, s->max_weight, s->d.ncols};
    for (int i = 0; i < 4; ++i) info[i] = v[i];
    return QD_OK;
}

extern "C" int qd_parity_counts(const qd_calib *s, const uint64_t *d_planes, int64_t plane_stride, int64_t nwords, int64_t *d_counts, void *stream)
{
    if (!s) return qd_fail(QD_EINVAL, "null column table");
    if (nwords < 0) return qd_fail(QD_EINVAL, "negative word count");
    if (nwords > QD_CALIB_MAX_WORDS) return qd_fail(QD_EINVAL, "%lld words: at most 2^25 (2^31 shots) in one call", (long long)nwords);
    if (plane_stride < nwords) return qd_fail(QD_EINVAL, "plane_stride %lld is smaller than the %lld words of a plane", (long long)plane_stride, (long long)nwords);
    if (nwords == 0 || s->d.ntasks == 0) return QD_OK;
    if (!d_planes || !d_counts) return qd_fail(QD_EINVAL, "null planes or counters");
    HIP_TRY(hipSetDevice(s->device));
    hipLaunchKernelGGL(qd_parity_counts_kernel, dim3(calib_blocks(s->d.ntasks)), dim3(QD_CALIB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), s->d,
                       reinterpret_cast<const u64 *>(d_planes), plane_stride, nwords, reinterpret_cast<long long *>(d_counts));
    HIP_TRY(hipGetLastError());
    return QD_OK;
}
