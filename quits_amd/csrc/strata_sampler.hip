// strata_sampler.hip -- the stratified DEM sampler (qd_strata_create, qd_strata_destroy, qd_strata_info, qd_sample_dem_strata): shots of the
// detector error model conditioned on exactly k faults firing.  The law, the random stream and the threshold table are stated in
// quits_amd/strata.py, whose sample_mirror is this kernel's specification; no reference counterpart (Stim draws independent faults only).
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#define QD_STRATA_LDS_MAX (64 * 1024)   // detector and observable bits of the 64 shots of a wavefront
#define QD_STRATA_STREAM 2u             // last Philox counter word (qd_sample_dem: 0, qd_sample_circuit: 1)

// One wavefront per workgroup, one lane per shot.  The walk over the faults is sequential in r (the faults still to place), so a shot cannot be
// spread over lanes; instead the 64 shots of a wavefront walk j together:
//   * j, and with it the Philox counter word, the rows of Ht / Lt and every loop bound, is the same in all lanes: the loops and their branches
//     are wave-uniform, the CSR rows are read at one address for the whole wavefront, and only `inc` (this lane includes fault j) predicates the LDS updates;
//   * the threshold q[j][r] is gathered by the lane's own r from row j of the table (kmax + 1 words: the lanes of one stratum sit a few
//     words apart, in one or two cache lines).  The four thresholds of a Philox group are fetched together with the r the lane has at the
//     head of the group; a lane that places a fault inside the group -- a few in a thousand -- fetches the later ones again;
//   * a lane's detector and observable bits are a column of LDS, word w at bits[64 w + lane]: no two lanes share a word (no atomics) and the
//     64 lanes of an update hit 64 consecutive words (no bank conflict).  Its fault bits are collected in a register and stored one word per
//     32 faults to its own row; the wavefront stops drawing once every lane has r = 0 and writes zero words from there on.
// The detector and observable bytes are written by the whole wavefront row by row (64 consecutive bytes per store), after a barrier that
// orders the LDS columns before the reads across them.  Plain vector loads and stores only.
__global__ void __launch_bounds__(QD_WAVE) qd_sample_strata_kernel(SpmatDev Ht, SpmatDev Lt, const uint32_t *__restrict__ thr, int kmax, uint32_t k0,
                                                                  uint32_t k1, int64_t shot0, const int64_t *__restrict__ shot_list,
                                                                  const int32_t *__restrict__ kk, int64_t B, int m, int nobs, uint8_t *det,
                                                                  int64_t det_stride, uint8_t *obs, int64_t obs_stride, uint32_t *fault_bits,
                                                                  int64_t fault_stride)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *bits = reinterpret_cast<uint32_t *>(smem);
    const int lane = threadIdx.x;
    const int dwords = (m + 31) >> 5, owords = (nobs + 31) >> 5;
    const int n = Ht.nrows, fwords = (n + 31) >> 5, K1 = kmax + 1;
    const int64_t b0 = (int64_t)blockIdx.x * QD_WAVE, b = b0 + lane;
    const bool live = b < B;
    for (int w = 0; w < dwords + owords; ++w) bits[w * QD_WAVE + lane] = 0u;
    const uint64_t shot = live ? (uint64_t)(shot_list ? shot_list[b] : shot0 + b) : 0ull;
    int r = live ? kk[b] : 0;
    r = r < 0 ? 0 : (r > kmax ? kmax : r);                  // a count outside 0 .. min(kmax, n) is clamped: the table has no such column,
    r = r > n ? n : r;                                      // and more than n faults cannot be placed
    uint32_t *frow = fault_bits + (live ? b : 0) * fault_stride;
    for (int w = 0; w < fwords; ++w) {
        uint32_t fw = 0u;
        if (__ballot(r > 0) != 0ull) {                      // (uniform) somebody still has faults to place
            for (int g = 0; g < 8 && 32 * w + 4 * g < n; ++g) {
                const int c = 8 * w + g;
                uint32_t rnd[4], t4[4];
                const int r0 = r;
#pragma unroll
                for (int x = 0; x < 4; ++x) t4[x] = 4 * c + x < n ? thr[(size_t)(4 * c + x) * K1 + r0] : 0u;
                qd_philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), (uint32_t)c, QD_STRATA_STREAM, k0, k1, rnd);
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int j = 4 * c + x;
                    uint32_t t = t4[x];
                    if (r != r0 && j < n) t = thr[(size_t)j * K1 + r];
                    const bool inc = j < n && r > 0 && (rnd[x] < t || n - j == r);
                    if (__ballot(inc) != 0ull) {            // (uniform) walk fault j's detectors and observables once for the lanes that include it
                        for (uint32_t e = Ht.row_ptr[j]; e < Ht.row_ptr[j + 1]; ++e) {
                            const uint32_t d = Ht.col_idx[e];
                            if (inc) bits[(d >> 5) * QD_WAVE + lane] ^= 1u << (d & 31u);
                        }
                        for (uint32_t e = Lt.row_ptr[j]; e < Lt.row_ptr[j + 1]; ++e) {
                            const uint32_t o = Lt.col_idx[e];
                            if (inc) bits[(dwords + (o >> 5)) * QD_WAVE + lane] ^= 1u << (o & 31u);
                        }
                    }
                    if (inc) {
                        fw |= 1u << (j & 31);
                        --r;
                    }
                }
            }
        }
        if (live) frow[w] = fw;
    }
    __syncthreads();
    const uint32_t *obits = bits + dwords * QD_WAVE;
    for (int l = 0; l < QD_WAVE && b0 + l < B; ++l) {      // (uniform) row b0 + l, written by all lanes
        for (int i = lane; i < m; i += QD_WAVE) det[(b0 + l) * det_stride + i] = (uint8_t)((bits[(i >> 5) * QD_WAVE + l] >> (i & 31)) & 1u);
        for (int i = lane; i < nobs; i += QD_WAVE) obs[(b0 + l) * obs_stride + i] = (uint8_t)((obits[(i >> 5) * QD_WAVE + l] >> (i & 31)) & 1u);
    }
}

hipError_t qd_launch_sample_strata(const SpmatDev &Ht, const SpmatDev &Lt, const uint32_t *thr, int kmax, uint64_t seed, int64_t shot0,
                                   const int64_t *shot_list, const int32_t *kk, int64_t B, int m, int nobs, uint8_t *det, int64_t det_stride,
                                   uint8_t *obs, int64_t obs_stride, uint32_t *fault_bits, int64_t fault_stride, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    const size_t lds = sizeof(uint32_t) * QD_WAVE * (size_t)(((m + 31) >> 5) + ((nobs + 31) >> 5));
    hipLaunchKernelGGL(qd_sample_strata_kernel, dim3((unsigned)((B + QD_WAVE - 1) / QD_WAVE)), dim3(QD_WAVE), lds, s, Ht, Lt, thr, kmax, (uint32_t)seed,
                       (uint32_t)(seed >> 32), shot0, shot_list, kk, B, m, nobs, det, det_stride, obs, obs_stride, fault_bits, fault_stride);
    return hipGetLastError();
}

extern "C" int qd_strata_create(int32_t n, int32_t kmax, const uint32_t *thresholds, int32_t device, qd_strata **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (n < 1) return qd_fail(QD_EINVAL, "n = %d: a model has at least one fault", n);
    if (kmax < 0 || kmax > QD_FAULT_HIST - 1) return qd_fail(QD_EINVAL, "kmax = %d outside 0 .. %d", kmax, QD_FAULT_HIST - 1);
    if (!thresholds) return qd_fail(QD_EINVAL, "null thresholds");
    const size_t K1 = (size_t)kmax + 1;
    for (int j = 0; j < n; ++j)
        if (thresholds[(size_t)j * K1] != 0u)
            return qd_fail(QD_EINVAL, "thresholds[%d][0] = %u: column 0 (nothing left to place) must be 0", j, thresholds[(size_t)j * K1]);
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    qd_strata *s = new qd_strata();
    s->device = device;
    s->n = n;
    s->kmax = kmax;
    s->thr = static_cast<const uint32_t *>(s->mem.upload(thresholds, sizeof(uint32_t) * (size_t)n * K1));
    if (!s->thr) { s->mem.release(); delete s; return qd_fail(QD_EHIP, "device allocation/upload failed"); }
    *out = s;
    return QD_OK;
}

extern "C" void qd_strata_destroy(qd_strata *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->mem.release();
    delete s;
}

extern "C" int qd_strata_info(const qd_strata *s, int64_t *info)
{
    if (!s || !info) return qd_fail(QD_EINVAL, "null argument");
    info[0] = s->n;
    info[1] = s->kmax;
    info[2] = (int64_t)sizeof(uint32_t) * s->n * (s->kmax + 1);
    info[3] = s->device;
    return QD_OK;
}

extern "C" int qd_sample_dem_strata(const qd_strata *strata, const qd_spmat *Ht, const qd_spmat *Lt, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                                    const int32_t *d_k, int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride,
                                    uint32_t *d_fault_bits, int64_t fault_stride_words, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || B > (int64_t)QD_WAVE * INT32_MAX) return qd_fail(QD_EINVAL, "bad shot count (negative, or more than 64 (2^31 - 1) in one call)");
    if (!d_shots && shot0 < 0) return qd_fail(QD_EINVAL, "negative shot0");
    if (!d_k) return qd_fail(QD_EINVAL, "null fault counts (d_k)");
    if (!strata || !Ht || !Lt || !d_det || !d_obs || !d_fault_bits) return qd_fail(QD_EINVAL, "null argument");
    if (Ht->d.nrows != Lt->d.nrows) return qd_fail(QD_EINVAL, "Ht and Lt must both have one row per fault");
    const int n = Ht->d.nrows, m = Ht->d.ncols, nobs = Lt->d.ncols;
    if (n != strata->n) return qd_fail(QD_EINVAL, "the threshold table is for %d faults, Ht has %d rows", strata->n, n);
    if (Ht->device != strata->device) return qd_fail(QD_EINVAL, "the threshold table is on device %d, Ht on device %d", strata->device, Ht->device);
    if (det_stride < m || obs_stride < nobs) return qd_fail(QD_EINVAL, "output strides too small");
    if (fault_stride_words * 32 < n) return qd_fail(QD_EINVAL, "fault rows hold %lld bits, the model has %d faults", (long long)fault_stride_words * 32, n);
    const int64_t lds = 4ll * QD_WAVE * (((int64_t)m + 31) / 32 + ((int64_t)nobs + 31) / 32);
    if (lds > QD_STRATA_LDS_MAX)
        return qd_fail(QD_ECAPACITY, "%d detectors and %d observables need %lld B of LDS per wavefront of 64 shots, budget %d B", m, nobs, (long long)lds,
                       QD_STRATA_LDS_MAX);
    HIP_TRY(hipSetDevice(strata->device));
    HIP_TRY(qd_launch_sample_strata(Ht->d, Lt->d, strata->thr, strata->kmax, seed, d_shots ? 0 : shot0, d_shots, d_k, B, m, nobs, d_det, det_stride, d_obs,
                                    obs_stride, d_fault_bits, fault_stride_words, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}
