// frame_sampler.hip -- circuit-level detector sampler (qd_sample_circuit): a Pauli frame per shot propagated through the
// circuit, Stim's detector-sampler semantics without gauge randomisation (exact for deterministic detectors; quits_amd/frame.py
// states the rules, the random stream and the program layout; tests/frame_mirror.py is the CPU restatement).
//
// Layout.  One wavefront = 64 shots, one workgroup, nothing shared with any other wavefront.  Bit l of every 64-bit word is
// shot b0 + l.  LDS holds the X and Z frame words of every qubit, a ring of measurement-record words (slot = measurement
// index mod ring, resolved by the host) and the observable words.  The wave walks the program; each instruction is one step:
//   gates / measurements : lanes stride over the instruction's targets (the host split parts so that no qubit repeats);
//   noise                : lane l draws shot l's Philox words, four sites per call; __ballot turns the 64 fire decisions of a site
//                          into that site's flip mask, which lane 0 XORs into the target's frame word (ds_xor_b64); a Pauli channel
//                          picks its component by counting the cumulative thresholds not above the draw (frame.py: biased noise);
//   DETECTOR             : the XOR of its ring words (a broadcast read), kept by lane d mod 64 in a register;
//   FLUSH                : a block of <= 64 detectors -> bytes: 64 row stores, lane l writing detector base + l of row r;
//   OBSERVABLE_INCLUDE   : XOR into the observable's LDS word; written out as bytes at the end.
// One wavefront per workgroup, so __syncthreads() between steps only orders the LDS traffic of the wave.
#include "qd_internal.h"
#include "qd_host.h"

// The noise sites of one instruction.  thr: the threshold below which a site fires (for a Pauli channel its last cumulative
// threshold T_K).  tab: T_1 .. T_K of a Pauli channel (K = 3 / 15), unused otherwise; the address is the same in every lane and the
// data is never written while the kernel runs, so the table is read once per instruction with scalar loads and stays in SGPRs.
template <int OP>
__device__ __forceinline__ void qd_frame_noise(const int32_t *__restrict__ ins, int n, uint32_t thr, const QdUniformU32 *tab, uint32_t s_lo,
                                               uint32_t s_hi, uint32_t k0, uint32_t k1, uint64_t *FX, uint64_t *FZ, int lane)
{
    constexpr int K = OP == QD_FOP_PC1 ? 3 : (OP == QD_FOP_PC2 ? 15 : 1);
    uint32_t T[K];
    if (OP == QD_FOP_PC1 || OP == QD_FOP_PC2) {
#pragma unroll
        for (int k = 0; k < K - 1; ++k) T[k] = tab[k];
    }
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
            } else if (OP == QD_FOP_YERR) {
                const uint64_t m = __ballot(fire);
                if (lane == 0) {
                    atomicXor((unsigned long long *)(FX + q[j]), (unsigned long long)m);
                    atomicXor((unsigned long long *)(FZ + q[j]), (unsigned long long)m);
                }
            } else if (OP == QD_FOP_DEP1 || OP == QD_FOP_PC1) {
                uint32_t p = 1u;                                // 1 = X, 2 = Y, 3 = Z
                if (OP == QD_FOP_DEP1) p += r[x] % 3u;
                else {                                          // component = 1 + the number of thresholds T_1 .. T_{K-1} not above r
#pragma unroll
                    for (int k = 0; k < K - 1; ++k) p += r[x] >= T[k] ? 1u : 0u;
                }
                const uint64_t xm = __ballot(fire && p != 3u), zm = __ballot(fire && p != 1u);
                if (lane == 0) {
                    if (xm) atomicXor((unsigned long long *)(FX + q[j]), (unsigned long long)xm);
                    if (zm) atomicXor((unsigned long long *)(FZ + q[j]), (unsigned long long)zm);
                }
            } else {                                            // two-qubit: component v in 1 .. 15, first target v >> 2, second v & 3
                uint32_t v = 1u;
                if (OP == QD_FOP_DEP2) v += r[x] % 15u;
                else {
#pragma unroll
                    for (int k = 0; k < K - 1; ++k) v += r[x] >= T[k] ? 1u : 0u;
                }
                const uint32_t a = v >> 2, b = v & 3u;
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

// CHANNELS: the program holds Y_ERROR / PAULI_CHANNEL_1 / PAULI_CHANNEL_2 (FrameDev::channels, set by qd_circuit_create).  A program
// without them runs the instantiation that does not contain their code, i.e. the kernel it ran before these opcodes existed (34 VGPRs;
// with them 35 VGPRs, and a channel's table held in SGPRs across the Philox rounds).  The switch has no arm that leaves the loop: qd_circuit_create
// admits only the opcodes below, and an arm that set pc = prog_len made the compiler wrap every ds_xor_b64 of the noise sites in a
// wave reduction (v_mbcnt / s_bcnt1 / s_mul per XOR), 7 % on BB144 r12.
template <bool CHANNELS>
__global__ void __launch_bounds__(QD_WAVE) qd_frame_sample_kernel(FrameDev c, uint32_t k0, uint32_t k1, int64_t shot0,
                                                                   const int64_t *__restrict__ shot_list, int64_t B,
                                                                   uint8_t *__restrict__ det, int64_t det_stride,
                                                                   uint8_t *__restrict__ obs, int64_t obs_stride)
{
    extern __shared__ __align__(16) uint64_t fsm[];
    uint64_t *FX = fsm, *FZ = fsm + c.nq, *ring = FZ + c.nq, *ob = ring + c.ring;
    const int lane = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * QD_WAVE;
    const int rows = (int)min<int64_t>(QD_WAVE, B - b0);
    // row b0 + l is shot shot0 + b0 + l, or shot_list[b0 + l] (qd_sample_circuit_shots: any order, repeats allowed); a lane past the batch draws for a shot nobody reads
    const uint64_t shot = (uint64_t)(shot_list && lane < rows ? shot_list[b0 + lane] : shot0 + b0 + lane);
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
                if (op == QD_FOP_XERR) qd_frame_noise<QD_FOP_XERR>(ins, n, t, nullptr, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else if (op == QD_FOP_ZERR) qd_frame_noise<QD_FOP_ZERR>(ins, n, t, nullptr, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else if (op == QD_FOP_DEP1) qd_frame_noise<QD_FOP_DEP1>(ins, n, t, nullptr, s_lo, s_hi, k0, k1, FX, FZ, lane);
                else qd_frame_noise<QD_FOP_DEP2>(ins, n, t, nullptr, s_lo, s_hi, k0, k1, FX, FZ, lane);
            }
            pc += 4 + (op == QD_FOP_DEP2 ? 2 * n : n);
            break;
        }
        case QD_FOP_YERR:
            if constexpr (CHANNELS) {
                const uint32_t t = c.thr[ins[2]];
                if (t) qd_frame_noise<QD_FOP_YERR>(ins, n, t, nullptr, s_lo, s_hi, k0, k1, FX, FZ, lane);
                pc += 4 + n;
            } else __builtin_unreachable();
            break;
        case QD_FOP_PC1:                                        // thresholds ins[2] .. ins[2] + 2 are the channel's cumulative table
            if constexpr (CHANNELS) {
                const QdUniformU32 *tab = (const QdUniformU32 *)c.thr + ins[2];
                const uint32_t t = tab[2];
                if (t) qd_frame_noise<QD_FOP_PC1>(ins, n, t, tab, s_lo, s_hi, k0, k1, FX, FZ, lane);
                pc += 4 + n;
            } else __builtin_unreachable();
            break;
        case QD_FOP_PC2:                                        // ins[2] .. ins[2] + 14
            if constexpr (CHANNELS) {
                const QdUniformU32 *tab = (const QdUniformU32 *)c.thr + ins[2];
                const uint32_t t = tab[14];
                if (t) qd_frame_noise<QD_FOP_PC2>(ins, n, t, tab, s_lo, s_hi, k0, k1, FX, FZ, lane);
                pc += 4 + 2 * n;
            } else __builtin_unreachable();
            break;
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
        case QD_FOP_OBS: {
            uint64_t w = 0ull;
            for (int i = 0; i < n; ++i) w ^= ring[ins[3 + i]];
            if (lane == 0) ob[ins[2]] ^= w;
            pc += 3 + n;
            break;
        }
        default:                                                // qd_circuit_create admits no other opcode
            __builtin_unreachable();
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

hipError_t qd_launch_frame_sample(const FrameDev &c, uint64_t seed, int64_t shot0, const int64_t *shot_list, int64_t B, uint8_t *det,
                                  int64_t det_stride, uint8_t *obs, int64_t obs_stride, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((B + QD_WAVE - 1) / QD_WAVE));
    if (c.channels)
        hipLaunchKernelGGL(qd_frame_sample_kernel<true>, grid, dim3(QD_WAVE), (size_t)c.lds_bytes, s, c, (uint32_t)seed,
                           (uint32_t)(seed >> 32), shot0, shot_list, B, det, det_stride, obs, obs_stride);
    else
        hipLaunchKernelGGL(qd_frame_sample_kernel<false>, grid, dim3(QD_WAVE), (size_t)c.lds_bytes, s, c, (uint32_t)seed,
                           (uint32_t)(seed >> 32), shot0, shot_list, B, det, det_stride, obs, obs_stride);
    return hipGetLastError();
}
