"""Gradient bucketing with backward/communication overlap.

The reference overlapped parameter-server pushes with backward through its
dependency engine (per-key engine vars). The MI355X-native
equivalent: gradients accumulate directly into flat per-bucket buffers
(param.grad views), a post-accumulate hook fires an async RCCL all-reduce the
moment a bucket's last gradient lands, and `finish()` joins the outstanding
works before the optimizer step. Buckets are sized for xGMI ring collectives
(7 point-to-point links/GPU, ~153 GB/s each): default 50 MiB so RCCL's
multi-ring pipelining amortizes per-collective latency without delaying
overlap (override with DTMX_BUCKET_MB).

Buckets are filled in *reverse* parameter order — backward produces gradients
roughly last-layer-first, so reverse order makes buckets complete early and
overlap deepest (same reasoning as the reference's per-key ordering by sorted
keys, kvstore_nccl.h:213-318, re-derived for collectives).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist


# Elements per chunk of the segment tables; equals OPT_CHUNK of
# dtmx/csrc/optimizer.hip (checked against ext.opt_chunk() when tables are
# uploaded).
OPT_CHUNK = 4096


def build_segment_tables(sizes: Sequence[int], chunk: int = OPT_CHUNK) -> Dict[str, List[int]]:
    """Per-parameter ("segment") view of a flat bucket, as plain int lists.

    Segment s is the element range [seg_off[s], seg_off[s+1]) of the flat. It
    is cut into chunks of at most `chunk` consecutive elements, counted from
    the segment's start, so no chunk straddles two segments and a parameter's
    chunking depends on its own size only. chunk_start is an index into the
    flat; seg_chunk_off[s] is the first chunk of segment s (nseg+1 entries).
    A zero-size segment has no chunk."""
    assert chunk > 0
    seg_off, chunk_seg, chunk_start, chunk_len, seg_chunk_off = [0], [], [], [], [0]
    for s, n in enumerate(sizes):
        n = int(n)
        assert n >= 0
        base = seg_off[-1]
        for o in range(0, n, chunk):
            chunk_seg.append(s)
            chunk_start.append(base + o)
            chunk_len.append(min(chunk, n - o))
        seg_off.append(base + n)
        seg_chunk_off.append(len(chunk_seg))
    assert seg_off[-1] < 2 ** 31, "a flat bucket must hold fewer than 2^31 elements"
    return {"seg_off": seg_off, "chunk_seg": chunk_seg, "chunk_start": chunk_start,
            "chunk_len": chunk_len, "seg_chunk_off": seg_chunk_off}


class SegmentTables:
    """Device copy of build_segment_tables() for one bucket plus the persistent
    norm workspaces: part [nchunks][2] f32 per-chunk {sum master^2, sum g^2},
    sq [nseg][2] f64 per-segment sums, seg_lr [nseg] f32. Derived data, not
    optimizer state."""

    def __init__(self, sizes: Sequence[int], device, chunk: int = OPT_CHUNK):
        t = build_segment_tables(sizes, chunk)
        i32 = lambda v, dev: torch.tensor(v, dtype=torch.int32, device=dev)
        self.seg_off = i32(t["seg_off"], "cpu")       # host copy (validation)
        self.chunk_seg = i32(t["chunk_seg"], device)
        self.chunk_start = i32(t["chunk_start"], device)
        self.chunk_len = i32(t["chunk_len"], device)
        self.seg_chunk_off = i32(t["seg_chunk_off"], device)
        self.nseg, self.nchunks = len(sizes), len(t["chunk_seg"])
        self.part = torch.empty(self.nchunks, 2, dtype=torch.float32, device=device)
        self.sq = torch.zeros(self.nseg, 2, dtype=torch.float64, device=device)
        self.seg_lr = torch.zeros(self.nseg, dtype=torch.float32, device=device)


class GradBucketer:
    """With `flatten_params=True` the parameters themselves are also moved
    into per-bucket flat bf16 buffers (p.data becomes a [strided] view), plus
    fp32 master and momentum flats — so the whole optimizer step is ONE fused
    HIP kernel per bucket (dtmx/csrc/softmax_opt.hip sgd_mom_mp; for NAG and
    LBSGD dtmx/csrc/optimizer.hip, LBSGD with two small norm launches in
    front) instead of 2-4 torch ops per tensor (reference optimizer_op-inl.h
    MP_SGDMom redesign as a multi-tensor kernel)."""

    def __init__(self, params: Sequence[torch.nn.Parameter],
                 bucket_mb: Optional[float] = None, average: bool = False,
                 flatten_params: bool = False, async_mode: bool = False):
        """async_mode (kvstore 'dist_async'): the collective analog of the
        reference's asynchronous PS (kvstore_dist 'dist_async' — workers never
        barrier on each other's pushes). Gradients are double-buffered: step
        t's all-reduce completes in the background while step t+1 computes,
        and the optimizer consumes the one-step-delayed reduced gradients —
        full comm/compute overlap, staleness bounded at 1 step."""
        self.params = [p for p in params if p.requires_grad]
        self.average = average
        self.flatten_params = flatten_params
        self.async_mode = async_mode
        self.flat_w: List[torch.Tensor] = []
        self.flat_master: List[torch.Tensor] = []
        self.flat_mom: List[torch.Tensor] = []
        self._seg_tables: Optional[List[SegmentTables]] = None
        bucket_mb = bucket_mb or float(os.environ.get("DTMX_BUCKET_MB", "50"))
        bucket_bytes = int(bucket_mb * 1024 * 1024)

        # assign params to buckets in reverse order
        self.buckets: List[List[torch.nn.Parameter]] = []
        cur: List[torch.nn.Parameter] = []
        cur_bytes = 0
        for p in reversed(self.params):
            sz = p.numel() * p.element_size()
            if cur and cur_bytes + sz > bucket_bytes:
                self.buckets.append(cur)
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += sz
        if cur:
            self.buckets.append(cur)

        # flat buffers + grad views
        self.flat: List[torch.Tensor] = []
        self._param_bucket: Dict[int, int] = {}
        self._pending: List[int] = []
        self._works: List[Tuple[int, dist.Work]] = []
        for bi, bucket in enumerate(self.buckets):
            numel = sum(p.numel() for p in bucket)
            dev = bucket[0].device
            buf = torch.zeros(numel, dtype=bucket[0].dtype, device=dev)
            wbuf = None
            if self.flatten_params:
                wbuf = torch.empty(numel, dtype=bucket[0].dtype, device=dev)
            off = 0
            for p in bucket:
                n = p.numel()
                p.grad = self._shaped_view(buf, off, p)
                if wbuf is not None:
                    with torch.no_grad():
                        src = (
                            p.detach().permute(0, 2, 3, 1).reshape(-1)  # KRSC order
                            if p.dim() == 4 else p.detach().reshape(-1)
                        )
                        wbuf[off : off + n].copy_(src)
                        p.data = self._shaped_view(wbuf, off, p)
                off += n
                self._param_bucket[id(p)] = bi
            self.flat.append(buf)
            if wbuf is not None:
                self.flat_w.append(wbuf)
                self.flat_master.append(wbuf.detach().float())
                self.flat_mom.append(torch.zeros(numel, dtype=torch.float32, device=dev))
        self._pending = [len(b) for b in self.buckets]
        self._hooks = [
            p.register_post_accumulate_grad_hook(self._on_grad_ready) for p in self.params
        ]
        self._enabled = dist.is_initialized() and dist.get_world_size() > 1
        if self.async_mode:
            # shadow grad set: the accumulation/allreduce target alternates
            self.flat_shadow = [torch.zeros_like(b) for b in self.flat]
            self._views_main = [p.grad for p in self.params]
            # shadow views in self.params order
            vs = {}
            for bi, bucket in enumerate(self.buckets):
                off = 0
                for p in bucket:
                    vs[id(p)] = self._shaped_view(self.flat_shadow[bi], off, p)
                    off += p.numel()
            self._views_shadow = [vs[id(p)] for p in self.params]
            self._prev_works: List[Tuple[int, dist.Work]] = []
            self._cur_is_shadow = False

    @staticmethod
    def _shaped_view(buf: torch.Tensor, off: int, p: torch.Tensor) -> torch.Tensor:
        """View matching p's logical shape AND memory layout (channels_last
        for 4D conv weights) so flat bytes line up between w/grad/master."""
        v = buf[off : off + p.numel()]
        if p.dim() == 4:
            K, C, R, S = p.shape
            return v.view(K, R, S, C).permute(0, 3, 1, 2)
        return v.view(p.shape)

    # -- fused optimizer step ----------------------------------------------
    def fused_sgd_step(self, lr: float, momentum: float, wd: float,
                       rescale: float, clip: float = 0.0,
                       hyper: Optional[torch.Tensor] = None):
        """hyper: optional device float32[5] {lr,mom,wd,rescale,clip} — when
        given, the kernel reads hyperparameters from it (hipGraph-capturable:
        update the buffer between replays instead of re-recording)."""
        from ..ops.hip import require_ext

        ext = require_ext()
        grads = self.reduced_flats() if self.async_mode else self.flat
        for bi in range(len(self.flat)):
            if hyper is not None:
                ext.sgd_mom_mp_dev(self.flat_w[bi], grads[bi],
                                   self.flat_master[bi], self.flat_mom[bi], hyper)
            else:
                ext.sgd_mom_mp(self.flat_w[bi], grads[bi], self.flat_master[bi],
                               self.flat_mom[bi], lr, momentum, wd, rescale, clip)

    def segment_tables(self) -> List[SegmentTables]:
        """Per-bucket segment/chunk tables and norm workspaces, built on first
        use (only the LBSGD step needs them)."""
        if self._seg_tables is None:
            assert self.flatten_params, "segment tables need flatten_params=True"
            from ..ops.hip import require_ext

            assert require_ext().opt_chunk() == OPT_CHUNK
            self._seg_tables = [
                SegmentTables([p.numel() for p in bucket], self.flat_w[bi].device)
                for bi, bucket in enumerate(self.buckets)
            ]
        return self._seg_tables

    def fused_lbsgd_step(self, lr: float, momentum: float, wd: float,
                         rescale: float, clip: float = 0.0, eta: float = 0.001,
                         hyper: Optional[torch.Tensor] = None):
        """LBSGD on the flats: per bucket, two small launches reduce every
        parameter's |master|^2 and |g|^2 and write its trust-ratio learning
        rate (tables.seg_lr), then one launch applies the sgd_mom_mp body with
        that rate. `lr` already carries the warmup ramp. No host sync.
        hyper: optional device float32[6] {lr,mom,wd,rescale,clip,eta}, as in
        fused_sgd_step."""
        from ..ops.hip import require_ext

        ext = require_ext()
        grads = self.reduced_flats() if self.async_mode else self.flat
        tabs = self.segment_tables()
        for bi in range(len(self.flat)):
            t = tabs[bi]
            ext.seg_sqnorm(grads[bi], self.flat_master[bi], t.chunk_start,
                           t.chunk_len, t.seg_chunk_off, t.seg_off, t.part, t.sq,
                           t.seg_lr, lr, wd, rescale, clip, eta, hyper)
            if hyper is not None:
                ext.lbsgd_mom_mp_dev(self.flat_w[bi], grads[bi],
                                     self.flat_master[bi], self.flat_mom[bi],
                                     t.chunk_seg, t.chunk_start, t.chunk_len,
                                     t.seg_lr, t.seg_off, hyper)
            else:
                ext.lbsgd_mom_mp(self.flat_w[bi], grads[bi], self.flat_master[bi],
                                 self.flat_mom[bi], t.chunk_seg, t.chunk_start,
                                 t.chunk_len, t.seg_lr, t.seg_off, momentum, wd,
                                 rescale, clip)

    def fused_nag_step(self, lr: float, momentum: float, wd: float,
                       rescale: float, clip: float = 0.0,
                       hyper: Optional[torch.Tensor] = None):
        """Nesterov momentum on the flats, one launch per bucket. hyper as in
        fused_sgd_step (a sixth entry is ignored)."""
        from ..ops.hip import require_ext

        ext = require_ext()
        grads = self.reduced_flats() if self.async_mode else self.flat
        for bi in range(len(self.flat)):
            if hyper is not None:
                ext.nag_mom_mp_dev(self.flat_w[bi], grads[bi],
                                   self.flat_master[bi], self.flat_mom[bi], hyper)
            else:
                ext.nag_mom_mp(self.flat_w[bi], grads[bi], self.flat_master[bi],
                               self.flat_mom[bi], lr, momentum, wd, rescale, clip)

    def state_tensors(self) -> List[torch.Tensor]:
        return self.flat_w + self.flat_master + self.flat_mom

    # -- per-iteration lifecycle -------------------------------------------
    def zero_grad(self):
        if self.async_mode:
            # swap the accumulation target; the other set's all-reduce keeps
            # flying while this step computes
            self._cur_is_shadow = not self._cur_is_shadow
            views = self._views_shadow if self._cur_is_shadow else self._views_main
            for p, v in zip(self.params, views):
                p.grad = v
            for buf in self._cur_flats():
                buf.zero_()
            self._pending = [len(b) for b in self.buckets]
            return
        for buf in self.flat:
            buf.zero_()
        self._pending = [len(b) for b in self.buckets]
        self._works.clear()

    def _cur_flats(self):
        return self.flat_shadow if getattr(self, "_cur_is_shadow", False) else self.flat

    def reduced_flats(self):
        """async mode: the one-step-delayed, fully reduced gradient set."""
        return self.flat if self._cur_is_shadow else self.flat_shadow

    def reduced_views(self):
        return self._views_main if self._cur_is_shadow else self._views_shadow

    def _on_grad_ready(self, param: torch.nn.Parameter):
        bi = self._param_bucket[id(param)]
        self._pending[bi] -= 1
        if self._pending[bi] == 0 and self._enabled:
            flat = self._cur_flats()[bi] if self.async_mode else self.flat[bi]
            if getattr(self, "_gc_residual", None) is not None and flat.is_cuda:
                self._compressed_reduce(bi)
            else:
                work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, async_op=True)
                self._works.append((bi, work))

    def finish(self):
        """Join outstanding collectives; call before the optimizer step.
        async mode: joins the PREVIOUS step's collectives (usually already
        complete) and rotates the work queues — the optimizer then reads
        reduced_flats()/reduced_views()."""
        if self.async_mode:
            for bi, work in self._prev_works:
                work.wait()
            self._prev_works = self._works
            self._works = []
            return
        for bi, work in self._works:
            work.wait()
            if self.average:
                self.flat[bi].div_(dist.get_world_size())
        self._works.clear()

    # -- 2-bit compressed reduction (reference gradient compression over
    # collectives: quantize w/ error feedback -> all-gather the packed codes
    # -> local dequantize-sum; the server dequantized before merging
    # (kvstore_dist_server.h:606), so the numerics match; wire bytes drop
    # ~8x (2 bits vs bf16), per-GPU traffic ~2x lower at world=8) --
    def set_compression(self, threshold: float):
        self._gc_threshold = float(threshold)
        self._gc_residual = [
            torch.zeros_like(b, dtype=torch.float32) for b in self.flat
        ]

    def _compressed_reduce(self, bi: int):
        from ..ops.hip import require_ext

        ext = require_ext()
        world = dist.get_world_size()
        # async mode accumulates into the shadow set — reduce THAT buffer,
        # not the in-flight previous-step one (self.flat[bi] would be stale).
        flat = self._cur_flats()[bi] if self.async_mode else self.flat[bi]
        packed = ext.quantize_2bit(flat.view(-1), self._gc_residual[bi].view(-1),
                                   self._gc_threshold)
        gathered = [torch.empty_like(packed) for _ in range(world)]
        dist.all_gather(gathered, packed)
        out = ext.dequantize_2bit(gathered[0], flat.numel(), self._gc_threshold)
        for g in gathered[1:]:
            out += ext.dequantize_2bit(g, flat.numel(), self._gc_threshold)
        if self.average:
            # finish() only averages buckets with outstanding works; the
            # compressed path completes synchronously, so average here.
            out /= world
        flat.view(-1).copy_(out)

    def rebuild_after_membership_change(self):
        """Communicator changed (elastic re-form): nothing to re-shard in the
        replicated-DP layout; hooks and buffers stay valid, only the process
        group changed. Re-read world size lazily in finish()."""
        self._enabled = dist.is_initialized() and dist.get_world_size() > 1

    def detach(self):
        for h in self._hooks:
            h.remove()
        self._hooks.clear()
