// qd_sample.hip -- everything around the decoder: sparse GF(2) matrices and their products, the DEM and circuit samplers, and the flag and
// tally kernels of a memory experiment.
#include "qd_host.h"

#include <cmath>

extern "C" int qd_spmat_create(int32_t nrows, int32_t ncols, const int32_t *row_ptr, const int32_t *col_idx,
                               int32_t device, qd_spmat **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (nrows < 0 || ncols < 0 || !row_ptr) return qd_fail(QD_EINVAL, "bad shape");
    const int nnz = row_ptr[nrows];
    if (nnz > 0 && !col_idx) return qd_fail(QD_EINVAL, "null col_idx");
    for (int e = 0; e < nnz; ++e)
        if (col_idx[e] < 0 || col_idx[e] >= ncols) return qd_fail(QD_EINVAL, "column index out of range");
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    qd_spmat *s = new qd_spmat();
    s->device = device;
    std::vector<uint32_t> rp(row_ptr, row_ptr + nrows + 1), ci(col_idx, col_idx + nnz);
    int rc = s->mem.upload(rp, &s->d.row_ptr) | s->mem.upload(ci, &s->d.col_idx);
    if (rc) { s->mem.release(); delete s; return qd_fail(QD_EHIP, "device allocation/upload failed"); }
    s->d.nrows = nrows; s->d.ncols = ncols; s->d.nnz = nnz;
    s->d.colmask = nullptr; s->d.mask_words = 0;
    if (nrows > 0 && nrows <= 512 && ncols > 0) {
        const int mw = (nrows + 31) / 32;
        std::vector<uint32_t> cm((size_t)ncols * mw, 0u);
        for (int r = 0; r < nrows; ++r)
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) cm[(size_t)col_idx[e] * mw + (r >> 5)] ^= 1u << (r & 31);
        if (s->mem.upload(cm, &s->d.colmask)) { s->mem.release(); delete s; return qd_fail(QD_EHIP, "device allocation/upload failed"); }
        s->d.mask_words = mw;
    }
    *out = s;
    return QD_OK;
}

extern "C" void qd_spmat_destroy(qd_spmat *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->mem.release();
    delete s;
}

extern "C" int qd_gf2_spmv_batch(const qd_spmat *A, const uint32_t *d_err_bits, int64_t err_stride_words, int64_t B,
                                 uint8_t *d_out, int64_t out_stride, int32_t accumulate, void *stream)
{
    if (!A || !d_err_bits || !d_out) return qd_fail(QD_EINVAL, "null argument");
    if (err_stride_words * 32 < A->d.ncols) return qd_fail(QD_EINVAL, "error rows hold %lld bits, matrix has %d columns", (long long)err_stride_words * 32, A->d.ncols);
    if (out_stride < A->d.nrows) return qd_fail(QD_EINVAL, "out_stride smaller than the row count");
    HIP_TRY(hipSetDevice(A->device));
    HIP_TRY(qd_launch_spmv(A->d, d_err_bits, err_stride_words, B, d_out, out_stride, accumulate, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_unpack_bits(const uint32_t *d_bits, int64_t stride_words, int32_t nbits, int64_t B, uint8_t *d_out,
                              int64_t out_stride, void *stream)
{
    if (!d_bits || !d_out || nbits < 0 || stride_words * 32 < nbits || out_stride < nbits) return qd_fail(QD_EINVAL, "bad unpack arguments");
    HIP_TRY(qd_launch_unpack(d_bits, stride_words, nbits, B, d_out, out_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_count_mismatch(const uint8_t *d_pred, const uint8_t *d_obs, int32_t k, int64_t B, int64_t *d_count,
                                 void *stream)
{
    if (!d_pred || !d_obs || !d_count || k <= 0) return qd_fail(QD_EINVAL, "bad count arguments");
    HIP_TRY(qd_launch_count(d_pred, d_obs, k, B, d_count, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

// qd_sample_dem (d_shots == nullptr: shots shot0 .. shot0 + B - 1) and qd_sample_dem_shots (row b = shot d_shots[b])
int qd_sample_dem_impl(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                       int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, uint32_t *d_fault_bits,
                       int64_t fault_stride_words, void *stream)
{
    if (!Ht || !Lt || !priors || !d_det || !d_obs) return qd_fail(QD_EINVAL, "null argument");
    if (Ht->d.nrows != Lt->d.nrows) return qd_fail(QD_EINVAL, "Ht and Lt must both have one row per fault");
    const int n = Ht->d.nrows, m = Ht->d.ncols, nobs = Lt->d.ncols;
    if (det_stride < m || obs_stride < nobs) return qd_fail(QD_EINVAL, "output strides too small");
    if (d_fault_bits && fault_stride_words * 32 < n) return qd_fail(QD_EINVAL, "fault rows hold %lld bits, the model has %d faults", (long long)fault_stride_words * 32, n);
    if (((m + 31) / 32 + (nobs + 31) / 32) * 4 > QD_SAMPLE_LDS_MAX) return qd_fail(QD_ECAPACITY, "too many detectors for the sampler's LDS bit array");
    HIP_TRY(hipSetDevice(Ht->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<uint32_t> thr((size_t)n);
    for (int j = 0; j < n; ++j) {
        double t = std::floor(priors[j] * 4294967296.0);
        thr[j] = (uint32_t)std::min(std::max(t, 0.0), 4294967295.0);
    }
    uint32_t *d_thr = nullptr;
    HIP_TRY(hipMalloc((void **)&d_thr, sizeof(uint32_t) * (size_t)std::max(n, 4)));
    hipError_t e = hipMemcpy(d_thr, thr.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = d_fault_bits ? qd_launch_sample_faults(Ht->d, Lt->d, d_thr, seed, shot0, d_shots, B, m, nobs, d_det, det_stride, d_obs, obs_stride, d_fault_bits,
                                                   fault_stride_words, s)
                         : qd_launch_sample(Ht->d, Lt->d, d_thr, seed, shot0, d_shots, B, m, nobs, d_det, det_stride, d_obs, obs_stride, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_thr);
    if (e != hipSuccess) return qd_fail(QD_EHIP, "sampler: %s", hipGetErrorString(e));
    return QD_OK;
}

extern "C" int qd_sample_dem(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0,
                             int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride,
                             void *stream)
{
    return qd_sample_dem_impl(Ht, Lt, priors, seed, shot0, nullptr, B, d_det, det_stride, d_obs, obs_stride, nullptr, 0, stream);
}

extern "C" int qd_sample_dem_shots(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, const int64_t *d_shots,
                                   int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || B > INT32_MAX) return qd_fail(QD_EINVAL, "bad shot count (one workgroup per shot: at most 2^31 - 1 in one call)");
    if (!d_shots) return qd_fail(QD_EINVAL, "null shot list");
    return qd_sample_dem_impl(Ht, Lt, priors, seed, 0, d_shots, B, d_det, det_stride, d_obs, obs_stride, nullptr, 0, stream);
}

// ---- circuit-level sampler (frame_sampler.hip): the program comes from quits_amd/frame.py; everything the kernel indexes with is
// checked here once, so the kernel trusts the program.
static int frame_check_program(const int32_t *p, int64_t len, int nq, int nmeas, int ndet, int nobs, const uint32_t *thr, int nthr, int ring,
                               int64_t *nsites, int *channels)
{
    *channels = 0;
    std::vector<int64_t> seen((size_t)nq, -1);     // qubit -> pc of the last gate part that used it
    int64_t pc = 0, sites = 0, meas = 0;
    int next_det = 0;
    auto bad = [&](const char *what) { return qd_fail(QD_EINVAL, "circuit program word %lld: %s", (long long)pc, what); };
    while (pc < len) {
        if (len - pc < 2) return bad("truncated instruction");
        const int op = p[pc], n = p[pc + 1];
        if (op < 0 || op >= QD_FOP_COUNT) return bad("unknown opcode");
        if (n < 0) return bad("negative count");
        int64_t width;
        switch (op) {
        case QD_FOP_R: case QD_FOP_H: width = 2 + (int64_t)n; break;
        case QD_FOP_CX: case QD_FOP_M: case QD_FOP_MX: case QD_FOP_MR: width = 2 + 2 * (int64_t)n; break;
        case QD_FOP_XERR: case QD_FOP_ZERR: case QD_FOP_DEP1: case QD_FOP_YERR: case QD_FOP_PC1: width = 4 + (int64_t)n; break;
        case QD_FOP_DEP2: case QD_FOP_PC2: width = 4 + 2 * (int64_t)n; break;
        case QD_FOP_FLUSH: width = 3; break;
        default: width = 3 + (int64_t)n; break;                 // DET, OBS
        }
        if (width > len - pc) return bad("instruction runs past the end of the program");
        const int32_t *a = p + pc + 2;
        if (op <= QD_FOP_MR) {
            const int per = (op == QD_FOP_R || op == QD_FOP_H) ? 1 : 2;
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < (op == QD_FOP_CX ? 2 : 1); ++k) {
                    const int q = a[per * i + k];
                    if (q < 0 || q >= nq) return bad("qubit out of range");
                    if (seen[q] == pc) return bad("a qubit repeats inside one gate part");
                    seen[q] = pc;
                }
            if (op >= QD_FOP_M) {
                for (int i = 0; i < n; ++i)
                    if (a[2 * i + 1] < 0 || a[2 * i + 1] >= ring) return bad("ring slot out of range");
                meas += n;
            }
        } else if (op <= QD_FOP_DEP2 || op >= QD_FOP_YERR) {
            if (op >= QD_FOP_YERR) *channels = 1;
            const int K = op == QD_FOP_PC1 ? 3 : (op == QD_FOP_PC2 ? 15 : 1);      // thresholds the instruction reads: a[0] .. a[0] + K - 1
            if (a[0] < 0 || a[0] >= nthr) return bad("threshold index out of range");
            if ((int64_t)a[0] + K > nthr) return bad("threshold table runs past the end of the thresholds");
            for (int k = 1; k < K; ++k)
                if (thr[a[0] + k] < thr[a[0] + k - 1]) return bad("threshold table must be non-decreasing (cumulative)");
            if (a[1] < 0 || (a[1] & 3)) return bad("first site must be a non-negative multiple of 4");
            const bool pairs = op == QD_FOP_DEP2 || op == QD_FOP_PC2;
            const int nt = pairs ? 2 * n : n;
            for (int i = 0; i < nt; ++i)
                if (a[2 + i] < 0 || a[2 + i] >= nq) return bad("qubit out of range");
            if (op == QD_FOP_PC2)
                for (int i = 0; i < n; ++i)
                    if (a[2 + 2 * i] == a[3 + 2 * i]) return bad("the two targets of a pair must differ");
            sites += n;
        } else if (op == QD_FOP_FLUSH) {
            if (n < 1 || n > QD_WAVE || a[0] < 0 || (a[0] & (QD_WAVE - 1)) || a[0] + n > ndet) return bad("bad detector block");
            if (a[0] + n != next_det) return bad("a flush must close the detector block just produced");
        } else {
            if (op == QD_FOP_DET) {
                if (a[0] != next_det) return bad("detectors must come in order");
                ++next_det;
            } else if (a[0] < 0 || a[0] >= nobs) return bad("observable out of range");
            for (int i = 0; i < n; ++i)
                if (a[1 + i] < 0 || a[1 + i] >= ring) return bad("ring slot out of range");
        }
        pc += width;
    }
    if (meas != nmeas) return qd_fail(QD_EINVAL, "program measures %lld times, nmeas = %d", (long long)meas, nmeas);
    if (next_det != ndet) return qd_fail(QD_EINVAL, "program defines %d detectors, ndet = %d", next_det, ndet);
    *nsites = sites;
    return QD_OK;
}

extern "C" int qd_circuit_create(const int32_t *program, int64_t program_len, int32_t nq, int32_t nmeas, int32_t ndet, int32_t nobs,
                                 const uint32_t *thresholds, int32_t nthr, int32_t max_lookback, int32_t device, qd_circuit **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (!program || program_len < 0 || program_len > INT32_MAX) return qd_fail(QD_EINVAL, "bad program");
    if (nq < 0 || nmeas < 0 || ndet < 0 || nobs < 0 || nthr < 0 || max_lookback < 1) return qd_fail(QD_EINVAL, "bad sizes");
    if (nthr > 0 && !thresholds) return qd_fail(QD_EINVAL, "null thresholds");
    const int64_t lds = 8 * (2 * (int64_t)nq + max_lookback + nobs);
    if (lds > QD_FRAME_LDS_MAX)
        return qd_fail(QD_ECAPACITY, "circuit needs %lld B of LDS per wavefront (%d qubits, %d-measurement ring, %d observables), budget %d B",
                    (long long)lds, nq, max_lookback, nobs, QD_FRAME_LDS_MAX);
    int64_t nsites = 0;
    int channels = 0;
    int rc = frame_check_program(program, program_len, nq, nmeas, ndet, nobs, thresholds, nthr, max_lookback, &nsites, &channels);
    if (rc) return rc;
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    qd_circuit *c = new qd_circuit();
    c->device = device;
    std::vector<int32_t> prog(program, program + program_len);
    std::vector<uint32_t> thr(thresholds, thresholds + nthr);
    if (c->mem.upload(prog, &c->d.prog) || c->mem.upload(thr, &c->d.thr)) {
        c->mem.release(); delete c; return qd_fail(QD_EHIP, "device allocation/upload failed");
    }
    c->d.prog_len = (int)program_len; c->d.nq = nq; c->d.ring = max_lookback; c->d.nobs = nobs; c->d.lds_bytes = (int)lds;
    c->d.channels = channels;
    c->nq = nq; c->nmeas = nmeas; c->ndet = ndet; c->nobs = nobs; c->nsites = nsites;
    *out = c;
    return QD_OK;
}

extern "C" void qd_circuit_destroy(qd_circuit *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->mem.release();
    delete c;
}

extern "C" int qd_circuit_info(const qd_circuit *c, int64_t *info)
{
    if (!c || !info) return qd_fail(QD_EINVAL, "null argument");
    const int64_t v[8] = {c->nq, c->nsites, c->d.lds_bytes, c->nmeas, c->ndet, c->nobs, c->d.ring, c->d.prog_len};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return QD_OK;
}

extern "C" int qd_sample_circuit(const qd_circuit *c, uint64_t seed, int64_t shot0, int64_t B, uint8_t *d_det, int64_t det_stride,
                                 uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (!c) return qd_fail(QD_EINVAL, "null circuit");
    if (B < 0 || shot0 < 0) return qd_fail(QD_EINVAL, "negative shot count or shot0");
    if (B > (int64_t)QD_WAVE * INT32_MAX) return qd_fail(QD_EINVAL, "too many shots in one call");
    if ((c->ndet > 0 && !d_det) || (c->nobs > 0 && !d_obs)) return qd_fail(QD_EINVAL, "null output");
    if (det_stride < c->ndet || obs_stride < c->nobs) return qd_fail(QD_EINVAL, "output strides too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(qd_launch_frame_sample(c->d, seed, shot0, nullptr, B, d_det, det_stride, d_obs, obs_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_sample_circuit_shots(const qd_circuit *c, uint64_t seed, const int64_t *d_shots, int64_t B, uint8_t *d_det, int64_t det_stride,
                                       uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (!c) return qd_fail(QD_EINVAL, "null circuit");
    if (B < 0) return qd_fail(QD_EINVAL, "negative shot count");
    if (B > (int64_t)QD_WAVE * INT32_MAX) return qd_fail(QD_EINVAL, "too many shots in one call");
    if (!d_shots) return qd_fail(QD_EINVAL, "null shot list");
    if ((c->ndet > 0 && !d_det) || (c->nobs > 0 && !d_obs)) return qd_fail(QD_EINVAL, "null output");
    if (det_stride < c->ndet || obs_stride < c->nobs) return qd_fail(QD_EINVAL, "output strides too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(qd_launch_frame_sample(c->d, seed, 0, d_shots, B, d_det, det_stride, d_obs, obs_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

// ---- the memory experiment's bookkeeping (experiment.hip)
extern "C" int qd_shot_flags_fold(const int32_t *d_status, int64_t B, uint8_t *d_flags, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return qd_fail(QD_EINVAL, "negative shot count");
    if (!d_status || !d_flags) return qd_fail(QD_EINVAL, "null status or flags");
    if (B > 256ll * INT32_MAX) return qd_fail(QD_EINVAL, "too many shots in one call");
    HIP_TRY(qd_launch_shot_flags(d_status, B, d_flags, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_tally_batch(const uint8_t *d_pred, int64_t pred_stride, const uint8_t *d_obs, int64_t obs_stride, int32_t k, int64_t B,
                              const uint8_t *d_flags, int64_t *d_counts, uint64_t *d_fail_mask, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return qd_fail(QD_EINVAL, "negative shot count");
    if (!d_pred || !d_obs || !d_counts) return qd_fail(QD_EINVAL, "null predictions, observables or counts");
    if (k <= 0 || k > QD_TALLY_MAX_K) return qd_fail(QD_EINVAL, "k = %d observables outside 1 .. %d", k, QD_TALLY_MAX_K);
    if (pred_stride < k || obs_stride < k) return qd_fail(QD_EINVAL, "row strides smaller than k");
    HIP_TRY(qd_launch_tally(d_pred, pred_stride, d_obs, obs_stride, k, B, d_flags, d_counts, d_fail_mask, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}
