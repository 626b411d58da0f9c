"""The two-stream driver of a DeviceWindowPlan (calls of two or more chunks) and the staging of host samples through it."""
from __future__ import annotations

import numpy as np


def _to_device_samples(zcheck_samples):
    import torch
    from ..samples import PackedSamples
    if isinstance(zcheck_samples, PackedSamples):              # bit-packed rows: moved as they are, widened on the device (qd_unpack_b8)
        ps = zcheck_samples
        if not ps.is_cuda:
            lo, hi = ps.bit0 >> 3, (ps.bit0 + ps.num_bits + 7) >> 3
            ps = PackedSamples(torch.from_numpy(np.ascontiguousarray(ps.data[:, lo:hi])).to("cuda"), ps.num_bits, ps.bit0 & 7)
        return ps.unpack()
    if isinstance(zcheck_samples, torch.Tensor):
        t = zcheck_samples
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        elif t.dtype != torch.uint8:
            t = torch.remainder(t, 2).to(torch.uint8)
        return t.to("cuda").contiguous()
    a = np.asarray(zcheck_samples)
    if a.dtype != np.uint8:
        a = (a % 2).astype(np.uint8) if a.dtype != np.bool_ else a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def correction_words_to_packed(words, nfaults):
    """int32 numpy [N, >= ceil(nfaults / 32)] of correction words -> host PackedSamples of nfaults bits: the library's little-endian words are
    Stim's b8 bytes as they are (bit j of a shot is bit j & 7 of byte j >> 3)."""
    from ..samples import PackedSamples
    w = np.ascontiguousarray(words).astype("<i4", copy=False)
    return PackedSamples(w.view(np.uint8).reshape(w.shape[0], 4 * w.shape[1])[:, :max((nfaults + 7) // 8, 0)], nfaults)


def lane_groups(nchunks, lanes):
    """Chunks of a call dealt to groups of at most `lanes`, as few groups as possible and as even as they come: 4 chunks on three lanes are 2 + 2,
    not 3 + 1 (a chunk alone overlaps nothing), 16 on three are 3 + 3 + 3 + 3 + 2 + 2."""
    if nchunks <= 0:
        return []
    ngrp = (nchunks + lanes - 1) // lanes
    return [nchunks // ngrp + (1 if g < nchunks % ngrp else 0) for g in range(ngrp)]


class TwoStreams:
    """What the two-stream driver keeps per plan, made at its first call: the BP stream and the post stream (on the device of the data; a
    high-priority post stream measured no different, profiles/r03x_post_stream_priority_ab.txt) and, between begin() and end(), the state
    of one call or of one chain of calls: a buffer of error words and one of hand-off syndromes per lane, the status table, every lane's
    last post-stage event, and the predictions handed out to a caller that has not synchronised yet."""

    def __init__(self, device):
        import torch
        self.s_bp = torch.cuda.Stream(device=device)
        self.s_post = torch.cuda.Stream(device=device)
        self.end()

    def begin(self, plan, device, stats_shots=None):
        """Fresh lane buffers for the plan's current lanes and chunk, allocated on the caller's stream.  stats_shots: the caller collects
        status words, so every window gets a row of that many of them; None: one row, a chunk per lane, written over and over."""
        import torch
        lanes, C, nwin = int(plan.lanes), plan.chunk, len(plan.windows)
        words = max(w["graph"].words for w in plan.windows)
        self.err = [torch.empty((C * words,), dtype=torch.int32, device=device) for _ in range(lanes)]
        self.upd = [torch.empty((C, plan.nz), dtype=torch.uint8, device=device) for _ in range(lanes)] if nwin > 1 else [None] * lanes
        self.status = torch.empty((1, lanes * C) if stats_shots is None else (nwin, stats_shots), dtype=torch.int32, device=device)
        self.post_done = [None] * lanes
        self.keep = []

    def end(self):
        self.err = self.upd = self.status = None
        self.post_done, self.keep = [], []

    def synchronize(self):
        self.s_bp.synchronize()
        self.s_post.synchronize()


def decode_pipelined(plan, det, stats, ready=None, correction=None, soft=None):
    """Calls of two or more chunks: the BP stages run on one side stream, the post-processing (OSD / LSD over the shots BP
    parked, acc ^= L e, the hand-off U e) on a second one, so that a chunk's post-processing runs beside the BP of the other
    chunks of its group -- the post-processors are chains of dependent steps that leave most issue slots of a CU idle, BP fills
    them (profiles/r03x_overlap_probe.txt, r03x_pipelined_driver_ab.txt).  Chunks are taken `plan.lanes` at a time (lanes A, B, ...,
    each with its own set of decoders = workspaces, plan.lane_decoders), windows outer inside a group:

        BP stream:    BP(A, 0)  BP(B, 0)    BP(A, 1)    BP(B, 1)   ...
        post stream:            post(A, 0)  post(B, 0)  post(A, 1) ...

    BP(X, k) waits for post(X, k - 1) (its syndrome needs that hand-off; it also frees the lane's buffers and decoder), post(X, k)
    for BP(X, k); both streams are in order.  Both start after everything queued on the caller's stream so far (inputs, the
    zeroed accumulator); the caller's stream resumes after the last post stage, which by stream order is after all the others.
    Every buffer is allocated on the caller's stream before the side streams start and none is released before that point.

    `ready` (decode_host_samples): one event per chunk of `det`, the chunk's host-to-device copy.  The call is then a link of a chain that
    the caller opened with plan.two_streams(device).begin(...): the lanes carry over from the call before, so that the BP stream of piece
    i + 1 starts behind its INPUT and the lanes, not behind piece i's last post stage.  The caller's stream is not made to wait at all and
    the result is not joined: the caller queues what it wants behind the post stream, synchronises the side streams itself when it has
    queued everything, and then calls end() (profiles/r06_host_chain_ab.txt).

    `correction`: DeviceWindowPlan.decode's; zero-filled on the caller's stream ahead of the side streams' start, then every window's
    committed bits are laid into it on the post stream, behind that window's acc ^= L e.

    `soft`: DeviceWindowPlan.decode's (it needs `correction`); zero-filled like it, then every window's status words are folded into it on the
    post stream behind that window's stage 2, and the chunk's correction is weighed behind its last window's committed bits."""
    import torch
    lane_decs = plan.lane_decoders()
    ts = plan.two_streams(det.device)
    s_bp, s_post = ts.s_bp, ts.s_post
    N, C, NL = det.shape[0], plan.chunk, int(plan.lanes)
    cur = torch.cuda.current_stream()
    pred = torch.zeros((N, plan.nobs), dtype=torch.uint8, device=det.device)
    if correction is not None:
        from .device import commit_bits
        plan.check_correction(correction, N, det.device)
        correction.zero_()
    if soft is not None:
        from .device import soft_fold, soft_weigh
        plan.check_soft(soft, correction, N, det.device)
        weights = plan.commit_weights()
        soft.zero_()
    if ready is None:
        ts.begin(plan, det.device, N if stats is not None else None)
    else:
        ts.keep.append(pred)               # nothing handed out may go back to the allocator before the caller has synchronised
    start = torch.cuda.Event()
    start.record(cur)                      # (the zeroed accumulator, the buffers)
    s_bp.wait_event(start)
    s_post.wait_event(start)
    post_done = ts.post_done
    try:
        ch0 = 0
        # groups of up to NL chunks, as even as they come (4 chunks on three lanes: 2 + 2, not 3 + 1 -- a chunk alone overlaps nothing)
        for gsz in lane_groups((N + C - 1) // C, NL):
            lanes = [(lane, (ch0 + lane) * C) for lane in range(gsz)]
            ch0 += gsz
            for k, w in enumerate(plan.windows):
                for lane, c0 in lanes:
                    d = lane_decs[k][lane]
                    chunk, acc = det[c0:c0 + C], pred[c0:c0 + C]
                    B = chunk.shape[0]
                    err = ts.err[lane][:B * w["graph"].words].view(B, w["graph"].words)
                    st = ts.status[k, c0:c0 + B] if stats is not None else ts.status[0, lane * C:lane * C + B]
                    upd = ts.upd[lane][:B] if k > 0 else None
                    if post_done[lane] is not None:
                        s_bp.wait_event(post_done[lane])
                    if ready is not None and k == 0:
                        s_bp.wait_event(ready[c0 // C])    # (the post stream follows through bp_done)
                    d.decode(chunk, w["row0"], upd, err_bits=err, status=st, stage=1, stream=s_bp)
                    bp_done = torch.cuda.Event()
                    bp_done.record(s_bp)
                    d.post_head_start(s_bp)            # (heavy post-processing gets onto the CUs before the next BP kernel fills them; decided on the device)
                    s_post.wait_event(bp_done)
                    d.decode(chunk, w["row0"], upd, err_bits=err, status=st, stage=2, stream=s_post)
                    if soft is not None:
                        soft_fold(st, soft[c0:c0 + C], stream=s_post)
                    w["L"].xor_apply(err, acc, accumulate=True, stream=s_post)
                    if correction is not None:
                        commit_bits(err, w["ncommit"], correction[c0:c0 + C], w["col0"], stream=s_post)
                        if soft is not None and k == len(plan.windows) - 1:
                            soft_weigh(correction[c0:c0 + C], plan.nfaults, weights, chunk, soft[c0:c0 + C], stream=s_post)
                    if w["U"] is not None:
                        w["U"].xor_apply(err, ts.upd[lane][:B], accumulate=False, stream=s_post)
                    post_done[lane] = torch.cuda.Event()
                    post_done[lane].record(s_post)
                    if stats is not None:
                        stats.append((k, st))
    except BaseException:
        # the buffers above were allocated on the caller's stream and are in use on the side streams: nothing may be handed back
        # to the allocator while queued kernels still write to them
        ts.synchronize()
        raise
    if ready is None:
        for e in post_done:
            if e is not None:
                cur.wait_event(e)
        ts.end()
    return pred


class HostStaging:
    """decode_host's buffers, per plan: two pinned and two device buffers of detector rows (one pair is filled while the other is decoded),
    the copy stream, the pinned output.  They only grow; how a call cuts its samples into pieces is the plan's business, not theirs."""

    def __init__(self, device):
        import torch
        self.device = device
        self.copy = torch.cuda.Stream(device=device)
        self.pin = self.dev = self.out = None
        self.pin_packed = self.dev_packed = None               # bit-packed rows on their way to `dev` (PackedSamples input)
        self.corr = self.corr_out = None                       # corrections wanted: two device buffers of correction words, the pinned output

    def fit_corrections(self, rows, shots, words):
        import torch
        if self.corr is None or self.corr[0].shape[1] != words or self.corr[0].shape[0] < rows:
            self.corr = [torch.empty((rows, words), dtype=torch.int32, device=self.device) for _ in range(2)]
        if self.corr_out is None or self.corr_out.shape[1] != words or self.corr_out.shape[0] < shots:
            self.corr_out = torch.empty((shots, words), dtype=torch.int32, pin_memory=True)

    def fit(self, rows, ndet, shots, nobs, packed_bytes=0):
        """packed_bytes > 0: the host rows arrive bit-packed, that many bytes each: the pinned buffers (and their device copies) are cut for
        them, [rows, packed_bytes], and only the device buffers hold a byte per detector."""
        import torch
        if packed_bytes:
            if self.pin_packed is None or self.pin_packed[0].shape[1] != packed_bytes or self.pin_packed[0].shape[0] < rows:
                self.pin_packed = [torch.empty((rows, packed_bytes), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
                self.dev_packed = [torch.empty((rows, packed_bytes), dtype=torch.uint8, device=self.device) for _ in range(2)]
            if self.dev is None or self.dev[0].shape[1] != ndet or self.dev[0].shape[0] < rows:
                self.pin = None
                self.dev = [torch.empty((rows, ndet), dtype=torch.uint8, device=self.device) for _ in range(2)]
        elif self.pin is None or self.pin[0].shape[1] != ndet or self.pin[0].shape[0] < rows:
            self.pin = [torch.empty((rows, ndet), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self.dev = [torch.empty((rows, ndet), dtype=torch.uint8, device=self.device) for _ in range(2)]
        if self.out is None or self.out.shape[0] < shots:
            self.out = torch.empty((shots, nobs), dtype=torch.uint8, pin_memory=True)


def decode_host_samples(plan, stage, a, corrections=False):
    """a: numpy [N, ndet], N > 0, any integer dtype or bool  ->  int64 numpy [N, nobs], through `stage` (a HostStaging): pieces of
    `plan.host_piece` shots, rounded down to whole chunks, are copied chunk by chunk into a pinned buffer and on to the device on the copy
    stream, beside the decoding of the piece before.  `a` may be host PackedSamples: then the PACKED rows are staged and copied, and
    qd_unpack_b8 on the copy stream fills the device buffer ahead of the event the decode waits for.
    corrections=True: returns (predictions, host PackedSamples of plan.nfaults bits): every piece is decoded with a device buffer of correction
    words (one per staging buffer) that leaves for a pinned buffer behind the piece's predictions."""
    import torch
    from ..samples import PackedSamples, unpack_b8_into
    N, ndet = a.shape
    packed = isinstance(a, PackedSamples)
    if packed:
        byte_lo, byte_hi, bit_lo = a.bit0 >> 3, (a.bit0 + a.num_bits + 7) >> 3, a.bit0 & 7
        rows_packed = a.data
    as_u8 = None if packed else (lambda x: x.view(np.uint8)) if a.dtype == np.bool_ else ((lambda x: x) if a.dtype == np.uint8 else (lambda x: (x % 2).astype(np.uint8)))
    piece = N if N <= plan.chunk else min(N, max(plan.chunk, int(plan.host_piece) // plan.chunk * plan.chunk))
    stage.fit(piece, ndet, N, plan.nobs, packed_bytes=(byte_hi - byte_lo) if packed else 0)
    out = stage.out
    cwords = (plan.nfaults + 31) // 32
    if corrections:
        stage.fit_corrections(piece, N, cwords)
        res_corr = np.empty((N, cwords), dtype=np.int32)
    cur = torch.cuda.current_stream()

    def collect(lo_, hi_):                                     # a finished piece: widened / copied here, beside the decoding of the next one
        res[lo_:hi_] = out[lo_:hi_].numpy()
        if corrections:
            res_corr[lo_:hi_] = stage.corr_out[lo_:hi_].numpy()
    h2d_done, dec_done = [None, None], [None, None]
    # calls of two or more chunks: the pieces go through the two-stream driver as ONE chain: the lanes carry over from piece to piece, a piece's BP
    # starts behind its own host-to-device copy, its predictions leave on the post stream; the caller's stream only waits at the very end
    # (0.958 -> 0.987 of the device-resident rate, profiles/r06_host_chain_ab.txt).  Plans with `pipeline` off and shorter calls: piece after piece
    # on the caller's stream
    chained = plan.pipeline and N >= 2 * plan.chunk
    ts = None
    res = np.empty((N, plan.nobs), dtype=np.int64)
    span = [None, None]                                        # the rows of `out` that the piece in flight on a lane will fill
    try:
        if chained:
            ts = plan.two_streams(stage.device)
            ts.begin(plan, stage.device)
        for i, lo in enumerate(range(0, N, piece)):
            hi = min(N, lo + piece)
            b = i & 1
            if h2d_done[b] is not None:
                h2d_done[b].synchronize()                      # the staging buffer has left for the GPU
            if dec_done[b] is not None:
                dec_done[b].synchronize()                      # the device buffer has been decoded, its predictions are in `out`:
                collect(*span[b])
            span[b] = (lo, hi)
            ready = []
            with torch.cuda.stream(stage.copy):                # chunk by chunk: the first chunk's BP starts behind ITS copy, not the piece's
                for c0 in range(0, hi - lo, plan.chunk):
                    c1 = min(hi - lo, c0 + plan.chunk)
                    if packed:
                        np.copyto(stage.pin_packed[b][c0:c1].numpy(), rows_packed[lo + c0:lo + c1, byte_lo:byte_hi])
                        stage.dev_packed[b][c0:c1].copy_(stage.pin_packed[b][c0:c1], non_blocking=True)
                        unpack_b8_into(stage.dev_packed[b][c0:c1], bit_lo, ndet, stage.dev[b][c0:c1], stream=stage.copy)
                    else:
                        np.copyto(stage.pin[b][c0:c1].numpy(), as_u8(a[lo + c0:lo + c1]))
                        stage.dev[b][c0:c1].copy_(stage.pin[b][c0:c1], non_blocking=True)
                    ready.append(torch.cuda.Event())
                    ready[-1].record(stage.copy)
            h2d_done[b] = ready[-1]
            dec_done[b] = torch.cuda.Event()
            if chained:                                        # (a ragged last piece too, whatever its size: it runs beside the piece before it)
                corr = stage.corr[b][:hi - lo] if corrections else None
                pred = (decode_pipelined(plan, stage.dev[b][:hi - lo], None, ready) if corr is None else
                        decode_pipelined(plan, stage.dev[b][:hi - lo], None, ready, correction=corr))
                with torch.cuda.stream(ts.s_post):             # (in order behind the piece's post stages)
                    out[lo:hi].copy_(pred, non_blocking=True)
                    if corrections:
                        stage.corr_out[lo:hi].copy_(corr, non_blocking=True)
                    dec_done[b].record(ts.s_post)
            else:
                cur.wait_event(h2d_done[b])
                corr = stage.corr[b][:hi - lo] if corrections else None
                pred = plan.decode(stage.dev[b][:hi - lo]) if corr is None else plan.decode(stage.dev[b][:hi - lo], None, corr)
                out[lo:hi].copy_(pred, non_blocking=True)
                if corrections:
                    stage.corr_out[lo:hi].copy_(corr, non_blocking=True)
                dec_done[b].record(cur)
    finally:
        if ts is not None:
            ts.synchronize()
            ts.end()
        cur.synchronize()
        stage.copy.synchronize()
    for b in (0, 1):
        if span[b] is not None:
            collect(*span[b])
    return (res, correction_words_to_packed(res_corr, plan.nfaults)) if corrections else res
