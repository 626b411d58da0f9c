// frame_sampler.hip -- circuit-level detector sampler (qd_sample_circuit): a Pauli frame per shot propagated through the
// circuit, Stim's detector-sampler semantics without gauge randomisation (exact for deterministic detectors; quits_amd/frame.py
// states the rules, the random stream and the program layout; tests/frame_mirror.py is the CPU restatement).
//
// Layout.  One wavefront = 64 shots, one workgroup, nothing shared with any other wavefront.  Bit l of every 64-bit word is
// shot b0 + l.  LDS holds the X and Z frame words of every qubit, a ring of measurement-record words (slot = measurement
// index mod ring, resolved by the host) and the observable words.  The wave walks the program; each instruction is one step:
//   gates / measurements : lanes stride over the instruction's targets (the host split parts so that no qubit repeats);
//   noise                : lane l draws shot l's Philox words, four sites per call; __ballot turns the 64 fire decisions of a site
//                          into that site's flip mask, which lane 0 XORs into the target's frame word (ds_xor_b64);
//   DETECTOR             : the XOR of its ring words (a broadcast read), kept by lane d mod 64 in a register;
//   FLUSH                : a block of <= 64 detectors -> bytes: 64 row stores, lane l writing detector base + l of row r;
//   OBSERVABLE_INCLUDE   : XOR into the observable's LDS word; written out as bytes at the end.
// One wavefront per workgroup, so __syncthreads() between steps only orders the LDS traffic of the wave.
#include "qd_internal.h"

template <int OP>
__device__ __forceinline__ void qd_frame_noise(const int32_t *__restrict__ ins, int n, uint32_t thr, uint32_t s_lo, uint32_t s_hi,
                                               uint32_t k0, uint32_t k1, uint64_t *FX, uint64_t *FZ, int lane)
{
    const uint32_t g0 = (uint32_t)ins[3] >> 2;          // first site, a multiple of 4
    const int32_t *q = ins + 4;
    for (int j0 = 0; j0 < n; j0 += 4) {
        uint32_t r[4];
        qd_philox4x32_10(s_lo, s_hi, g0 + (uint32_t)(j0 >> 2), 1u, k0, k1, r);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int j = j0 + x;
            if (j >= n) break;
            const bool fire = r[x] < thr;
            if (!__ballot(fire)) continue;
            if (OP == QD_FOP_XERR || OP == QD_FOP_ZERR) {
                const uint64_t m = __ballot(fire);
                if (lane == 0) atomicXor((unsigned long long *)((OP == QD_FOP_XERR ? FX : FZ) + q[j]), (unsigned long long)m);
            } else if (OP == QD_FOP_DEP1) {
                const uint32_t p = 1u + r[x] % 3u;              // 1 = X, 2 = Y, 3 = Z
                const uint64_t xm = __ballot(fire && p != 3u), zm = __ballot(fire && p != 1u);
                if (lane == 0) {
                    if (xm) atomicXor((unsigned long long *)(FX + q[j]), (unsigned long long)xm);
                    if (zm) atomicXor((unsigned long long *)(FZ + q[j]), (unsigned long long)zm);
                }
            } else {                                            // DEPOLARIZE2: v = 1 + r mod 15, first target v >> 2, second v & 3
                const uint32_t v = 1u + r[x] % 15u, a = v >> 2, b = v & 3u;
                const uint64_t xa = __ballot(fire && (a == 1u || a == 2u)), za = __ballot(fire && a >= 2u);
                const uint64_t xb = __ballot(fire && (b == 1u || b == 2u)), zb = __ballot(fire && b >= 2u);
                if (lane == 0) {
                    const int qa = q[2 * j], qb = q[2 * j + 1];
                    if (xa) atomicXor((unsigned long long *)(FX + qa), (unsigned long long)xa);
                    if (za) atomicXor((unsigned long long *)(FZ + qa), (unsigned long long)za);
                    if (xb) atomicXor((unsigned long long *)(FX + qb), (unsigned long long)xb);
                    if (zb) atomicXor((unsigned long long *)(FZ + qb), (unsigned long long)zb);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(QD_WAVE) qd_frame_sample_kernel(FrameDev c, uint32_t k0, uint32_t k1, int64_t shot0, int64_t B,
                                                                   uint8_t *__restrict__ det, int64_t det_stride,
                                                                   uint8_t *__restrict__ obs, int64_t obs_stride)
{
    extern __shared__ __align__(16) uint64_t fsm[];
    uint64_t *FX = fsm, *FZ = fsm + c.nq, *ring = FZ + c.nq, *ob = ring + c.ring;
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * QD_WAVE;
    const int rows = (int)min<int64_t>(QD_WAVE, B - b0);
    const uint64_t shot = (uint64_t)(shot0 + b0 + lane);
    const uint32_t s_lo = (uint32_t)shot, s_hi = (uint32_t)(shot >> 32);
    for (int i = lane; i < 2 * c.nq + c.ring + c.nobs; i += QD_WAVE) fsm[i] = 0ull;
    __syncthreads();
    const int32_t *__restrict__ prog = c.prog;
    uint64_t dreg = 0ull;                                       // lane l: the word of detector (block base) + l
    int pc = 0;
    while (pc < c.prog_len) {
        const int op = prog[pc], n = prog[pc + 1];
        const int32_t *ins = prog + pc;
        switch (op) {
        case QD_FOP_R:
            for (int i = lane; i < n; i += QD_WAVE) { const int q = ins[2 + i]; FX[q] = 0ull; FZ[q] = 0ull; }
            pc += 2 + n;
            break;
        case QD_FOP_H:
            for (int i = lane; i < n; i += QD_WAVE) { const int q = ins[2 + i]; const uint64_t t = FX[q]; FX[q] = FZ[q]; FZ[q] = t; }
            pc += 2 + n;
            break;
        case QD_FOP_CX:
            for (int i = lane; i < n; i += QD_WAVE) {
                const int a = ins[2 + 2 * i], b = ins[3 + 2 * i];
                FX[b] ^= FX[a];
                FZ[a] ^= FZ[b];
            }
            pc += 2 + 2 * n;
            break;
        case QD_FOP_M:
        case QD_FOP_MX:
        case QD_FOP_MR:
            for (int i = lane; i < n; i += QD_WAVE) {
                const int q = ins[2 + 2 * i], s = ins[3 + 2 * i];
                ring[s] = op == QD_FOP_MX ? FZ[q] : FX[q];
                if (op == QD_FOP_MR) { FX[q] = 0ull; FZ[q] = 0ull; }
            }
            pc += 2 + 2 * n;
            break;
        case QD_FOP_XERR:
        case QD_FOP_ZERR:
        case QD_FOP_DEP1:
        case QD_FOP_DEP2: {
            const uint32_t t = c.thr[ins[2]];
            if (t) {                                            // p = 0: no site of this instruction can fire
                if (op == QD_FOP_XERR) qd_frame_noise<QD_FOP_XERR>(ins, n, t, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else if (op == QD_FOP_ZERR) qd_frame_noise<QD_FOP_ZERR>(ins, n, t, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else if (op == QD_FOP_DEP1) qd_frame_noise<QD_FOP_DEP1>(ins, n, t, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else qd_frame_noise<QD_FOP_DEP2>(ins, n, t, s_lo, s_hi, k0, k1, FX, FZ, lane);
            }
            pc += 4 + (op == QD_FOP_DEP2 ? 2 * n : n);
            break;
        }
        case QD_FOP_DET: {
            uint64_t w = 0ull;
            for (int i = 0; i < n; ++i) w ^= ring[ins[3 + i]];
            if (lane == (ins[2] & (QD_WAVE - 1))) dreg = w;
            pc += 3 + n;
            break;
        }
        case QD_FOP_FLUSH: {
            const int base = ins[2];
            if (lane < n)
                for (int r = 0; r < rows; ++r) det[(b0 + r) * det_stride + base + lane] = (uint8_t)((dreg >> r) & 1ull);
            pc += 3;
            break;
        }
        default: {                                              // QD_FOP_OBS (qd_circuit_create admits no other opcode)
            uint64_t w = 0ull;
            for (int i = 0; i < n; ++i) w ^= ring[ins[3 + i]];
            if (lane == 0) ob[ins[2]] ^= w;
            pc += 3 + n;
            break;
        }
        }
        __syncthreads();
    }
    for (int o0 = 0; o0 < c.nobs; o0 += QD_WAVE) {
        const int o = o0 + lane;
        if (o < c.nobs) {
            const uint64_t w = ob[o];
            for (int r = 0; r < rows; ++r) obs[(b0 + r) * obs_stride + o] = (uint8_t)((w >> r) & 1ull);
        }
    }
}

hipError_t qd_launch_frame_sample(const FrameDev &c, uint64_t seed, int64_t shot0, int64_t B, uint8_t *det, int64_t det_stride,
                                  uint8_t *obs, int64_t obs_stride, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(qd_frame_sample_kernel, dim3((unsigned)((B + QD_WAVE - 1) / QD_WAVE)), dim3(QD_WAVE), (size_t)c.lds_bytes, s, c,
                       (uint32_t)seed, (uint32_t)(seed >> 32), shot0, B, det, det_stride, obs, obs_stride);
    return hipGetLastError();
}
