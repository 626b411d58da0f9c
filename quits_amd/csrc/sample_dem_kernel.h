// sample_dem_kernel.h -- the DEM sampler's kernel, shared by qd_sample_dem / qd_sample_dem_shots (gf2_kernels.hip: FAULTS = 0) and
// qd_sample_dem_faults (faults.hip: FAULTS = 1, 2).
#pragma once
#include "qd_internal.h"

// ---- DEM sampler (stands in for stim's detector sampler, quits/simulation.py:23-27).  Same integer recipe as
// oq_sample_dem (oracle/qd_oracle.c): Philox4x32-10, key = seed, counter = (shot lo, shot hi, j / 4, 0); word j & 3
// fires fault j iff it is < floor(p_j * 2^32) (qd_philox4x32_10: qd_internal.h).  One workgroup per shot, detector/observable bits accumulated in LDS.
// FAULTS (qd_sample_dem_faults): 0 = the faults are not kept (qd_sample_dem, qd_sample_dem_shots); 1 = a bitmap of the n faults in LDS behind the
// detector and observable bits, streamed out in whole words; 2 = the three do not fit the LDS: the shot's row of fault_bits is zeroed here and
// every firing sets its bit there with a vector atomic (the workgroup owns the row: its own barrier orders the zeroes before the atomics).
template <int FAULTS>
__global__ void qd_sample_dem_kernel(SpmatDev Ht, SpmatDev Lt, const uint32_t *__restrict__ thr, uint32_t k0,
                                     uint32_t k1, int64_t shot0, const int64_t *__restrict__ shot_list, int m, int nobs, uint8_t *det,
                                     int64_t det_stride, uint8_t *obs, int64_t obs_stride, uint32_t *fault_bits, int64_t fault_stride)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *dbits = reinterpret_cast<uint32_t *>(smem);
    const int dwords = (m + 31) >> 5, owords = (nobs + 31) >> 5;
    uint32_t *obits = dbits + dwords;
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t b = blockIdx.x;
    const uint64_t shot = (uint64_t)(shot_list ? shot_list[b] : shot0 + b);     // (qd_sample_dem_shots: row b is shot shot_list[b])
    const int n = Ht.nrows;
    const int fwords = FAULTS ? (n + 31) >> 5 : 0;
    uint32_t *fbits = FAULTS == 1 ? obits + owords : (FAULTS == 2 ? fault_bits + b * fault_stride : nullptr);
    for (int w = tid; w < dwords + owords + (FAULTS == 1 ? fwords : 0); w += T) dbits[w] = 0u;
    if (FAULTS == 2)
        for (int w = tid; w < fwords; w += T) fbits[w] = 0u;
    __syncthreads();
    for (int c = tid; 4 * c < n; c += T) {
        uint32_t r[4];
        qd_philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), (uint32_t)c, 0u, k0, k1, r);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int j = 4 * c + x;
            if (j < n && r[x] < thr[j]) {
                for (uint32_t e = Ht.row_ptr[j]; e < Ht.row_ptr[j + 1]; ++e) {
                    const uint32_t d = Ht.col_idx[e];
                    atomicXor(&dbits[d >> 5], 1u << (d & 31u));
                }
                for (uint32_t e = Lt.row_ptr[j]; e < Lt.row_ptr[j + 1]; ++e) {
                    const uint32_t o = Lt.col_idx[e];
                    atomicXor(&obits[o >> 5], 1u << (o & 31u));
                }
                if (FAULTS) atomicOr(&fbits[j >> 5], 1u << (j & 31));
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < m; i += T) det[b * det_stride + i] = (uint8_t)((dbits[i >> 5] >> (i & 31)) & 1u);
    for (int i = tid; i < nobs; i += T) obs[b * obs_stride + i] = (uint8_t)((obits[i >> 5] >> (i & 31)) & 1u);
    if (FAULTS == 1)
        for (int w = tid; w < fwords; w += T) fault_bits[b * fault_stride + w] = fbits[w];
}
