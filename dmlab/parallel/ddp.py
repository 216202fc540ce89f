"""Bucketed, backward-overlapped data parallelism over RCCL (xGMI) / gloo.

The reference has no DDP: after a full ``loss.backward()`` it issues one blocking
``all_reduce`` per parameter and then ``/= ws`` (task2/dist_utils.py:39-42,
task3/dist_utils.py:40-46).  Here:

* Gradients live in ONE flat buffer (``Program.flat.grad``; for a plain
  ``nn.Module`` the reducer builds its own) laid out in the order backward
  produces them, so each bucket is a contiguous slice — RCCL reduces it in place,
  no pack/unpack copies.
* A bucket's all-reduce is launched (async, on the process group's comm stream,
  ordered after the producing kernels by a stream event) the moment its last
  gradient is written; the remaining backward layers keep the GPU busy while the
  bucket crosses xGMI.  The caller's stream waits for all buckets at the end of
  backward (``work.wait()`` is a device-side wait on RCCL, not a host sync).
* Averaging: ``ReduceOp.AVG`` when the backend supports it; otherwise SUM and
  the 1/ws factor is either folded into the fused optimiser (``fold_average_into``,
  zero extra passes) or applied per bucket.
* Bucket size: on MI355X a ring all-reduce is bound by one xGMI link per GPU
  (~153 GB/s of the 7), so buckets are sized large (default 25 MB fp32) to amortise
  RCCL launch latency; the first bucket is capped smaller (``first_bucket_mb``) so
  communication starts early in backward, and the LAST one too (``last_bucket_mb``):
  it can only launch when backward's final layers are done, so all of it is exposed —
  only the first layers' few gradients should wait for the end of backward.
* Optional bf16 gradient communication (``comm_dtype=torch.bfloat16``) halves
  the bytes on the links.  The cast targets a persistent flat communication buffer
  (allocated once), so the hooks allocate nothing and stay on the side stream.
* Optional int8 gradient compression with error feedback (``compress="q8"``,
  :mod:`dmlab.parallel.compress`): a finished bucket is quantised on the hook's stream into
  its slice of one persistent payload buffer and all-gathered asynchronously; the end of
  backward waits for the gather and decodes the mean of every rank's payload into the
  bucket's gradient slice on the main stream (about 1/3.94 of the fp32 bytes sent; every rank
  decodes the same bits).  All buffers are allocated at construction.  Runs on the Python
  bucket state machine; not combinable with ``comm_dtype`` or ``small_allreduce="xgmi"``.
* Optional top-k gradient sparsification with error feedback (``compress="topk"``,
  ``compress_keep=K``): the same bucket path with the other codec of that module.  Every
  2048-element block of a bucket sends its K largest entries of gradient + residual as
  (fp32 value, uint16 index) and carries the rest forward (K = 32: 1/42.7 of the fp32 bytes).
* Bucket hooks on the weight-gradient side stream (``side_stream_hooks``; default on with
  RCCL buckets, off with ``small_allreduce="xgmi"`` whose spinning kernel would block the
  side stream; ``DMLAB_DDP_SIDE_HOOKS=0/1`` forces either).  Off = the one-layer-lag scheme
  in which the main stream waits for each layer's weight gradients before its bucket
  launches.
* ``broadcast_buffers`` (default on, as torch DDP): rank 0's floating-point module buffers
  (BatchNorm running statistics) are broadcast once per training step (or every
  ``buffer_sync_every`` forwards), so the running statistics agree on every rank and a
  rank-0 checkpoint holds what every rank evaluates with.  The buffers are re-pointed into
  ONE flat tensor at construction (one in-place collective, no flatten/unflatten copies),
  and the broadcast is issued asynchronously at the first gradient hook of backward — the
  forward is done updating the statistics and backward never reads them — and waited for
  at the end of backward, so it overlaps backward instead of heading the next forward.
  ``num_batches_tracked`` advances identically on every rank and is not sent.  Nothing is broadcast when the wrapper switches to ``eval()`` (a rank-0-
  only evaluation must not enter a collective): to evaluate every rank with rank 0's final
  statistics, call :meth:`sync_buffers` on every rank first (the task scripts do, before
  their evaluation and checkpoint).  With ``buffer_sync_every > 1`` the statistics differ
  between syncs, so that call is required there; such a step cannot be graph-captured (the
  forward counter would not advance per replay: capture raises).
* ``force_comm`` (or ``DMLAB_DDP_FORCE_COMM=1``): at world size 1 with an initialised
  process group (a 1-rank RCCL communicator), run the full multi-rank path anyway — native
  reducer, bucket hooks, one collective per bucket, buffer broadcasts — so the RCCL code is
  exercised on a single GPU exactly as it runs on eight.
* ``small_allreduce="xgmi"``: buckets of at most ``small_cap_mb`` go through the
  one-shot xGMI peer-memory all-reduce (:mod:`dmlab.parallel.xgmi`, one kernel, no ring
  steps) instead of RCCL — the latency-bound case of the labs' LeNet (207 KB of grads).
  Raising ``small_cap_mb`` past the bucket size routes the large buckets too; those take
  the two-shot kernel (reduce-scatter + all-gather over all xGMI links at once) at >= 3
  ranks, or always with ``xgmi_algo="two_shot"``.
* The bucket state machine (per-bucket countdowns, collective launch, the end-of-
  backward wait / cast-back / average) runs in C++ (``dmlab._C.Reducer``,
  ``csrc/reducer.cpp``) against the c10d ProcessGroup directly; ``native=False`` keeps
  the equivalent Python implementation below (used when the extension is absent).
"""
from __future__ import annotations

import contextlib

import torch
import torch.distributed as dist
import torch.nn as nn

from . import env
from .comm import avg_supported, init_parameters


class _Bucket:
    __slots__ = ("lo", "hi", "params", "pending", "work", "comm_buf", "scaled", "cmp")

    def __init__(self, lo, hi, params):
        self.lo, self.hi, self.params = lo, hi, params
        self.pending = set(params)
        self.work = None
        self.comm_buf = None
        self.scaled = False
        self.cmp = None  # compress=...: (this rank's payload slice, [ws, bytes] gather slice)




class DistributedDataParallel(nn.Module):
    def __init__(self, module: nn.Module, bucket_cap_mb: float = 25.0,
                 first_bucket_mb: float = 4.0, last_bucket_mb: float = 2.0, comm_dtype=None,
                 broadcast_init: bool = True,
                 process_group=None, average: bool = True, small_allreduce: str | None = None,
                 small_cap_mb: float = 4.0, native: bool | None = None, xgmi_algo: str = "auto",
                 side_stream_hooks: bool | None = None, broadcast_buffers: bool = True,
                 buffer_sync_every: int = 1, force_comm: bool | None = None,
                 compress: str | None = None, error_feedback: bool = True,
                 compress_keep: int = 32):
        super().__init__()
        if compress not in (None, "q8", "topk"):
            raise ValueError("compress: None | 'q8' | 'topk'")
        if compress is not None and comm_dtype is not None:
            raise ValueError(f"compress={compress!r} sends its own payload format: it cannot be "
                             "combined with comm_dtype")
        if compress is not None and small_allreduce == "xgmi":
            raise ValueError(f"compress={compress!r} all-gathers its payload: it cannot be "
                             "combined with small_allreduce='xgmi'")
        if compress == "topk":
            from .compress import _check_keep

            compress_keep = _check_keep(compress_keep)
        self.compress = compress
        self.compress_keep = compress_keep
        self.compressor = None      # Q8Compressor / TopKCompressor (owns the residual)
        self._cmp_payload = None    # this rank's payloads, bucket after bucket
        self._cmp_gathered = None   # every rank's payloads: per bucket one [ws, bytes] block
        self.module = module
        self.ws = env.get_world_size()
        if force_comm is None:
            import os

            force_comm = os.environ.get("DMLAB_DDP_FORCE_COMM", "0") == "1"
        if force_comm and not env.is_initialized():
            raise RuntimeError("DDP(force_comm=True) needs an initialised process group "
                               "(e.g. a 1-rank 'nccl' group: env.init(backend='nccl'))")
        # communication is live at ws > 1, or at ONE rank when forced: a 1-rank RCCL group
        # then runs the whole multi-rank machinery (native reducer, bucket hooks on the side
        # stream, every bucket's collective, buffer broadcasts) on the one-GPU box
        self.comm_active = self.ws > 1 or bool(force_comm)
        self.pg = process_group
        self.comm_dtype = comm_dtype
        self.average = average
        self._use_avg = avg_supported() if self.comm_active else False
        self._fold = False  # 1/ws folded into the optimiser
        self.program = module if hasattr(module, "register_grad_hook") else None
        self._last_mb = last_bucket_mb
        if side_stream_hooks is None:
            import os

            # default: on with RCCL buckets (the collective is enqueued on RCCL's own stream);
            # off with the spinning xGMI kernel, which would sit on the weight-gradient stream
            # in front of every later weight gradient until the peers arrive (unmeasured at
            # 2-8 GPUs: ADVICE r2).  DMLAB_DDP_SIDE_HOOKS=0/1 forces either scheme.
            e = os.environ.get("DMLAB_DDP_SIDE_HOOKS")
            side_stream_hooks = (e != "0") if e is not None else small_allreduce != "xgmi"
        self.side_stream_hooks = bool(side_stream_hooks)
        # final-layer buckets issued on the main stream (asyncOp=False) -- RCCL only: gloo's
        # synchronous collective would block the host (DMLAB_DDP_TAIL_SYNC=0 disables)
        import os as _os

        self._tail_sync = (_os.environ.get("DMLAB_DDP_TAIL_SYNC", "1") != "0"
                           and dist.is_initialized()
                           and dist.get_backend(process_group) == "nccl")
        self._py_tail = False
        self.broadcast_buffers = bool(broadcast_buffers)
        self.buffer_sync_every = max(1, int(buffer_sync_every))
        self._fwd_count = 0
        self._bcast_bufs = [b for b in module.buffers()] if self.comm_active else []
        self._buf_flat = None      # floating buffers re-pointed into one flat tensor
        self._buf_state = None     # "due": broadcast at the next backward's first hook
        self._buf_work = None      # the in-flight asynchronous broadcast
        if self.comm_active and self.broadcast_buffers:
            self._flatten_buffers()
        if broadcast_init and self.comm_active:
            init_parameters(module, force=True)
        if self.program is not None:
            self._setup_program(bucket_cap_mb, first_bucket_mb)
        else:
            self._setup_generic(bucket_cap_mb, first_bucket_mb)
        self.buckets_launched = 0
        self._sync_enabled = True
        # optional callback at the end of backward COMPUTE, before the bucket waits
        # (PhaseTimer uses it to measure the communication left exposed after backward)
        self.on_compute_done = None
        self._xgmi = None
        if small_allreduce not in (None, "rccl", "xgmi"):
            raise ValueError("small_allreduce: None | 'rccl' | 'xgmi'")
        if small_allreduce == "xgmi" and self.comm_active:
            cap = int(small_cap_mb * 2**20 / 4)
            small = [b.hi - b.lo for b in self.buckets if b.hi - b.lo <= cap]
            if self.grad_buf.dtype == torch.float32 and self.grad_buf.is_cuda and small:
                from .xgmi import XGMIAllReduce

                self._xgmi = XGMIAllReduce(cap=max(small), group=self.pg, algo=xgmi_algo)
        self._native = None
        if compress is not None:
            # the compressed exchange runs on the Python bucket state machine below
            native = False
            if self.comm_active:
                self._setup_compress(error_feedback)
        if native is None:
            native = self.comm_active and _native_reducer_available()
        # persistent communication buffer of the low-precision gradient copy (no per-step
        # allocation: graph-capturable, and safe to fill on the side stream)
        self._comm_flat = None
        if self.comm_dtype is not None and self.comm_dtype != self.grad_buf.dtype and \
                self.comm_active:
            self._comm_flat = torch.empty(self.grad_buf.numel(), dtype=self.comm_dtype,
                                          device=self.grad_buf.device)
        if native and self.comm_active:
            self._build_native(small_cap_mb)

    # ------------------------------------------------------------------ compression
    def _setup_compress(self, error_feedback):
        """Every buffer of the compressed exchange, allocated once (a step allocates nothing,
        so it can be captured): the residual, this rank's payloads laid end to end, and per
        bucket one contiguous ``[ws, payload_bytes]`` block for the gathered payloads."""
        from .compress import make_compressor

        if self.grad_buf.dtype != torch.float32:
            raise ValueError(f"compress={self.compress!r} needs fp32 gradients")
        dev = self.grad_buf.device
        self.compressor = make_compressor(self.compress, self.grad_buf.numel(), dev,
                                          error_feedback, self.compress_keep)
        sizes = [self.compressor.payload_bytes(b.hi - b.lo) for b in self.buckets]
        total = sum(sizes)
        self._cmp_payload = torch.zeros(total, dtype=torch.uint8, device=dev)
        self._cmp_gathered = torch.zeros(self.ws * total, dtype=torch.uint8, device=dev)
        off = 0
        for b, nb in zip(self.buckets, sizes):
            b.cmp = (self._cmp_payload[off:off + nb],
                     self._cmp_gathered[self.ws * off:self.ws * (off + nb)].view(self.ws, nb))
            off += nb

    def _launch_compressed(self, b: _Bucket):
        """Encode on the current stream (the weight-gradient side stream under
        ``side_stream_hooks``), then gather every rank's payload asynchronously.  Always the
        asynchronous form: a compressed bucket never takes the main-stream tail branch."""
        payload, gathered = b.cmp
        self.compressor.encode(self.grad_buf[b.lo:b.hi], b.lo, payload)
        if dist.get_backend(self.pg) == "nccl":
            b.work = dist.all_gather_into_tensor(gathered, payload, group=self.pg, async_op=True)
        else:
            b.work = dist.all_gather(list(gathered.unbind(0)), payload, group=self.pg,
                                     async_op=True)
        self.buckets_launched += 1

    @property
    def comm_bytes_per_step(self) -> int:
        """Bytes this rank hands to the bucket collectives per step."""
        n = sum(b.hi - b.lo for b in self.buckets)
        if self._cmp_payload is not None:
            return self._cmp_payload.numel()
        if self._comm_flat is not None:
            return n * self._comm_flat.element_size()
        return n * self.grad_buf.element_size()

    def residual_state(self):
        """Every rank's error-feedback residual as one ``[ws, N]`` CPU tensor (a collective:
        call it on every rank), or None without a residual.  The residual differs per rank and
        is training state, so a checkpoint carries all of them."""
        if self.compressor is None or self.compressor.residual is None:
            return None
        r = self.compressor.residual
        rows = torch.empty((self.ws, r.numel()), dtype=r.dtype, device=r.device)
        if self.ws == 1:
            rows[0].copy_(r)
        elif dist.get_backend(self.pg) == "nccl":
            dist.all_gather_into_tensor(rows, r, group=self.pg)
        else:
            dist.all_gather(list(rows.unbind(0)), r, group=self.pg)
        return rows.cpu()

    def load_residual_state(self, rows) -> bool:
        """Restore this rank's residual from :meth:`residual_state` output.  Returns False
        (residual left as it is) when the world size or the buffer size differs."""
        if self.compressor is None or self.compressor.residual is None or rows is None:
            return False
        r = self.compressor.residual
        if tuple(rows.shape) != (self.ws, r.numel()):
            return False
        r.copy_(rows[env.get_rank()].to(r.device, r.dtype))
        return True

    # ------------------------------------------------------------------ native reducer
    def _avg_scale(self):
        return 1.0 / self.ws if (self.average and not self._fold and self.ws > 1) else 1.0

    def _build_native(self, small_cap_mb):
        from dmlab import _C
        from torch.distributed import distributed_c10d as c10d

        pg = self.pg if self.pg is not None else c10d._get_default_group()
        nparams = max(self._bucket_of_index) + 1 if self._bucket_of_index else 0
        param_bucket = [-1] * nparams
        bid = {id(b): k for k, b in enumerate(self.buckets)}
        for i, b in self._bucket_of_index.items():
            param_bucket[i] = bid[id(b)]
        bounds = []
        for b in self.buckets:
            bounds += [int(b.lo), int(b.hi)]
        layer_params = [list(lp) for lp in getattr(self, "_layer_params", [])]
        code = {None: 0, torch.bfloat16: 1, torch.float16: 2}
        if self.comm_dtype not in code:
            raise ValueError(f"comm_dtype {self.comm_dtype} not supported")
        small_fn = None
        if self._xgmi is not None:
            xg = self._xgmi

            def small_fn(view, scale):
                xg(view, scale=scale)
        self._native = _C.Reducer(self.grad_buf, bounds, param_bucket, layer_params, pg,
                                  bool(self._use_avg), self._avg_scale(),
                                  code[self.comm_dtype],
                                  self._xgmi.cap if self._xgmi is not None else 0, small_fn,
                                  self._comm_flat)
        # RCCL: every asynchronous collective of the group runs in order on one stream, so
        # the end of backward waits for the last one only (gloo waits per operation)
        self._native.set_single_wait(self._tail_sync)

    @property
    def buckets_launched(self):
        return self._native.launched_total if self._native is not None else self._py_launched

    @buckets_launched.setter
    def buckets_launched(self, v):
        self._py_launched = v

    # ------------------------------------------------------------------ layout
    def _make_buckets(self, sizes, cap, first, last_cap=None):
        """sizes: per-param padded (offset, numel) in flat order -> buckets of ids."""
        buckets, cur, lo, acc = [], [], None, 0
        limit = first
        for i, (off, n, end) in enumerate(sizes):
            if lo is None:
                lo = off
            cur.append(i)
            acc = end - lo
            if acc >= limit:
                buckets.append(_Bucket(lo, end, cur))
                cur, lo, limit = [], None, cap
        if cur:
            buckets.append(_Bucket(lo, sizes[cur[-1]][2], cur))
        # the LAST bucket launches when backward's final layers are done, so all of it is
        # exposed communication: cap it (split at a parameter boundary) so only the first
        # layers' few gradients wait for the end of backward
        last = buckets[-1] if buckets else None
        limit_last = last_cap
        if last is not None and limit_last and len(last.params) > 1 and \
                last.hi - last.lo > limit_last:
            keep = list(last.params)
            split = len(keep)
            while split > 1 and sizes[keep[-1]][2] - sizes[keep[split - 1]][0] <= limit_last:
                split -= 1
            split = max(split, 1)
            if split < len(keep):
                head, tl = keep[:split], keep[split:]
                buckets[-1] = _Bucket(last.lo, sizes[tl[0]][0], head)
                buckets.append(_Bucket(sizes[tl[0]][0], last.hi, tl))
        return buckets

    def _setup_program(self, cap_mb, first_mb):
        prog = self.program
        flat = prog.flat
        self.grad_buf = flat.grad
        sizes = []
        for i, p in enumerate(flat.params):
            off = flat.offsets[i]
            end = flat.offsets[i + 1] if i + 1 < len(flat.params) else flat.numel
            sizes.append((off, p.numel(), end))
        el = 4
        self.buckets = self._make_buckets(sizes, cap_mb * 2**20 / el, first_mb * 2**20 / el,
                                          self._last_mb * 2**20 / el)
        self._bucket_of = {}
        for b in self.buckets:
            for i in b.params:
                self._bucket_of[i] = b
        self._bucket_of_index = {i: self._bucket_of[i] for i in range(len(flat.params))
                                 if i in self._bucket_of}
        self._layer_params = [prog.layer_params(i) for i in range(len(prog.layers))]
        if self.comm_active:  # one rank: nothing to launch per layer (finalize still runs)
            # stream_ok: the bucket launches only enqueue collectives (or the xGMI kernel), and
            # the bf16 cast into the persistent communication buffer, on the current stream
            # layers whose hook completes a bucket (the only ones that enqueue a collective;
            # the first hook also issues the buffer broadcast, ordered on the main stream)
            done = set()
            left = {id(b): len(b.params) for b in self.buckets}
            for li in range(len(self._layer_params) - 1, -1, -1):
                for i in self._layer_params[li]:
                    b = self._bucket_of_index.get(i)
                    if b is not None:
                        left[id(b)] -= 1
                        if left[id(b)] == 0:
                            done.add(li)
            self._launch_layers = done
            prog.register_grad_hook(self._on_layer_done, stream_ok=self.side_stream_hooks,
                                    enqueues=lambda li: li in self._launch_layers
                                    or self._xgmi is not None or self._comm_flat is not None)
        prog.register_post_backward_hook(lambda _p: self._finalize())

    def _setup_generic(self, cap_mb, first_mb):
        params = [p for p in self.module.parameters() if p.requires_grad]
        params = params[::-1]  # backward produces grads roughly in reverse order
        self._gparams = params
        dev = params[0].device
        offs, off = [], 0
        for p in params:
            offs.append(off)
            off += (p.numel() + 63) // 64 * 64
        self.grad_buf = torch.zeros(max(off, 64), device=dev, dtype=params[0].dtype)
        self._goffs = offs
        sizes = [(offs[i], p.numel(), offs[i + 1] if i + 1 < len(params) else off)
                 for i, p in enumerate(params)]
        el = self.grad_buf.element_size()
        self.buckets = self._make_buckets(sizes, cap_mb * 2**20 / el, first_mb * 2**20 / el,
                                          self._last_mb * 2**20 / el)
        self._bucket_of = {}
        for b in self.buckets:
            for i in b.params:
                self._bucket_of[i] = b
        self._bucket_of_index = {i: self._bucket_of[i] for i in range(len(params))
                                 if i in self._bucket_of}
        self._final_queued = False
        for i, p in enumerate(params):
            p.register_post_accumulate_grad_hook(self._make_generic_hook(i))

    def _gview(self, i):
        p = self._gparams[i]
        o = self._goffs[i]
        return self.grad_buf[o:o + p.numel()].view_as(p)

    def _make_generic_hook(self, i):
        def hook(p):
            v = self._gview(i)
            if p.grad is None:
                return
            if p.grad.data_ptr() != v.data_ptr():
                v.copy_(p.grad)
                p.grad = v
            if not self._final_queued:
                self._final_queued = True
                torch.autograd.Variable._execution_engine.queue_callback(self._finalize)
            if self._buf_state == "due":
                self._launch_buffer_sync()
            self._mark_ready(i)
        return hook

    # ------------------------------------------------------------------ runtime
    def fold_average_into(self, optimizer):
        """Communicate with SUM and let the fused optimiser apply 1/ws for free."""
        if self.ws > 1 and self.average:
            optimizer.grad_scale = 1.0 / self.ws
            self._fold = True
            if self._native is not None:
                self._native.set_avg_scale(1.0)
        return optimizer

    def _launch(self, b: _Bucket):
        if b.work is not None or not self.comm_active:
            b.work = b.work or True
            return
        if b.cmp is not None:
            self._launch_compressed(b)
            return
        view = self.grad_buf[b.lo:b.hi]
        if self._xgmi is not None and self.comm_dtype is None and view.numel() <= self._xgmi.cap:
            # one stream-ordered kernel, averaging folded into its epilogue
            scale = 1.0 / self.ws if (self.average and not self._fold) else 1.0
            self._xgmi(view, scale=scale)
            b.work, b.scaled = True, True
            self.buckets_launched += 1
            return
        if self._comm_flat is not None:
            b.comm_buf = self._comm_flat[b.lo:b.hi]
            b.comm_buf.copy_(view)
            t = b.comm_buf
        else:
            t = view
        if self.average and not self._fold and self._use_avg:
            op = dist.ReduceOp.AVG
        else:
            op = dist.ReduceOp.SUM
        if getattr(self, "_py_tail", False):
            # on the current stream, no host synchronisation (ProcessGroupNCCL asyncOp=False);
            # ordered after the collectives still in flight on the communication stream (one
            # communicator must not run two at once on different streams)
            for ob in self.buckets:
                if ob.work is not None and ob.work is not True:
                    ob.work.wait()
                    ob.work = True
            if self._buf_work is not None:
                self._buf_work.wait()
                self._buf_work = None
            dist.all_reduce(t, op=op, group=self.pg, async_op=False)
            b.work = True
        else:
            b.work = dist.all_reduce(t, op=op, group=self.pg, async_op=True)
        self.buckets_launched += 1

    def _mark_ready(self, i):
        if not self._sync_enabled:
            return
        if self._native is not None:
            self._native.mark_ready(i)
            return
        b = self._bucket_of.get(i)
        if b is None:
            return
        b.pending.discard(i)
        if not b.pending:
            self._launch(b)

    def _on_layer_done(self, prog, layer_idx):
        if self._buf_state == "due":
            self._launch_buffer_sync()
        # the Program runs the final layer's hooks on the main stream after joining the
        # weight-gradient stream: the buckets they complete are issued on that stream itself
        # (no hop through the communication stream on the step's critical tail)
        tail = bool(getattr(prog, "tail_hook", False)) and self._tail_sync
        if self._native is not None:
            if self._sync_enabled:
                if tail:
                    # the broadcast is the only collective that may still run on the
                    # communication stream when no bucket went there (the reducer orders a sync
                    # launch after its own last asynchronous bucket)
                    if self._buf_work is not None and not self._native.has_async():
                        self._buf_work.wait()
                        self._buf_work = None
                    self._native.set_sync_launch(True)
                try:
                    self._native.mark_layer(layer_idx)
                finally:
                    if tail:
                        self._native.set_sync_launch(False)
            return
        self._py_tail = tail
        try:
            for i in self._layer_params[layer_idx]:
                self._mark_ready(i)
        finally:
            self._py_tail = False

    def _finalize(self):
        if self.on_compute_done is not None:
            self.on_compute_done()
        if self._buf_state is not None or self._buf_work is not None:
            if (self._buf_state is None and self._native is not None and self._sync_enabled
                    and self._native.has_async()):
                # the broadcast went first on the process group's communication stream; the
                # reducer's wait for its last bucket, later on that stream, covers it
                self._buf_work = None
            else:
                self._wait_buffer_sync()
        if not self._sync_enabled:
            if self.program is None:
                self._final_queued = False
            return
        if self._xgmi is not None:
            self._xgmi.poll()  # a timed-out peer raises here (asynchronously, no sync)
        if self._native is not None:
            self._native.finalize()
            if self.program is None:
                self._final_queued = False
            return
        scale = 1.0 / self.ws if (self.average and not self._fold and not self._use_avg) else None
        for b in self.buckets:
            if b.work is None:  # unused parameters: launch now
                self._launch(b)
        for b in self.buckets:
            if b.work is not None and b.work is not True:
                b.work.wait()
            view = self.grad_buf[b.lo:b.hi]
            if b.cmp is not None and b.work is not None:
                # decode every rank's payload into the gradient slice, in rank order
                c = 1.0 / self.ws if (self.average and not self._fold) else 1.0
                self.compressor.decode_mean(b.cmp[1], view, c)
                b.scaled = True
            if b.comm_buf is not None:
                view.copy_(b.comm_buf)
                b.comm_buf = None
            if scale is not None and self.comm_active and not b.scaled:
                view.mul_(scale)
            b.work, b.scaled = None, False
            b.pending = set(b.params)
        if self.program is None:
            self._final_queued = False

    def reduce_now(self):
        """Reduce the whole gradient buffer now (every bucket, then the end-of-backward
        wait / cast-back / average): for steps that produce all gradients outside the
        per-layer hooks, e.g. :class:`dmlab.models.lenet_fused.FusedLeNetStep`."""
        if not self.comm_active:
            return
        if self._native is not None and self._sync_enabled:
            for lp in range(len(getattr(self, "_layer_params", []))):
                self._native.mark_layer(lp)
        self._finalize()

    # ------------------------------------------------------------------ buffers
    def _flatten_buffers(self):
        """Re-point every floating-point module buffer (BN running mean / var) into ONE flat
        tensor so a buffer sync is a single in-place collective: no per-step flatten /
        unflatten copies (``_broadcast_coalesced`` costs ~60 copy launches per ResNet-18
        forward).  Integer buffers (``num_batches_tracked``) advance identically on every
        rank and are not broadcast on this path."""
        slots = [(m, n, b) for m in self.module.modules() for n, b in m._buffers.items()
                 if b is not None and b.is_floating_point()]
        if not slots or len({(b.dtype, b.device) for _, _, b in slots}) != 1:
            self._buf_flat = None
            return
        flat = torch.cat([b.detach().reshape(-1) for _, _, b in slots])
        o = 0
        for m, n, b in slots:
            m._buffers[n] = flat[o:o + b.numel()].view_as(b)
            o += b.numel()
        self._buf_flat = flat
        self._buf_slots = slots
        self._buf_ptrs = [m._buffers[n].data_ptr() for m, n, _ in slots]

    def _buffers_still_flat(self) -> bool:
        return self._buf_flat is not None and all(
            m._buffers.get(n) is not None and m._buffers[n].data_ptr() == p
            for (m, n, _), p in zip(self._buf_slots, self._buf_ptrs))

    def _pg(self):
        from torch.distributed import distributed_c10d as c10d

        return self.pg if self.pg is not None else c10d._get_default_group()

    def _launch_buffer_sync(self):
        """Start the flat buffer broadcast asynchronously: issued at the first hook of
        backward (the forward has finished updating the running statistics and nothing in
        backward reads them), waited for at the end of backward, so it overlaps the whole
        backward instead of sitting at the head of the next forward."""
        self._buf_state = None
        if self._buffers_still_flat():
            self._buf_work = dist.broadcast(self._buf_flat, 0, group=self.pg, async_op=True)
        else:
            self.sync_buffers()

    def _wait_buffer_sync(self):
        if self._buf_state == "due":  # a training forward without a backward through hooks
            self._launch_buffer_sync()
        if self._buf_work is not None:
            self._buf_work.wait()
            self._buf_work = None

    def sync_buffers(self):
        """Broadcast rank 0's module buffers to every rank now (one collective on the flat
        buffer, or coalesced per dtype when the buffers were re-allocated)."""
        if not self.comm_active or not self._bcast_bufs:
            return
        if self._buf_work is not None:
            self._buf_work.wait()
            self._buf_work = None
        if self._buffers_still_flat():
            dist.broadcast(self._buf_flat, 0, group=self.pg)
            return
        self._bcast_bufs = [b for b in self.module.buffers()]
        dist._broadcast_coalesced(self._pg(), self._bcast_bufs, 256 * 2**20, 0)

    def forward(self, *a, **kw):
        if self.broadcast_buffers and self._bcast_bufs and self.module.training and \
                torch.is_grad_enabled():
            if self.buffer_sync_every > 1 and torch.cuda.is_available() and \
                    torch.cuda.is_current_stream_capturing():
                # a captured graph replays whatever the capture recorded: the every-k-th
                # forward counter would not advance per replay
                raise ValueError("DDP buffer_sync_every > 1 cannot be graph-captured")
            if self._buf_state == "due" or self._buf_work is not None:
                self._wait_buffer_sync()  # the previous forward never reached a backward
            if self._fwd_count % self.buffer_sync_every == 0:
                self._buf_state = "due"
            self._fwd_count += 1
        return self.module(*a, **kw)

    def check(self):
        """Raise if the xGMI all-reduce reported a timed-out peer.  The per-step poll in
        ``_finalize`` sees a timeout one step late (it reads the flag asynchronously, after
        the optimiser may already have applied that step); call this at the end of training
        so a timeout in the final steps is not missed."""
        if self._xgmi is not None:
            self._xgmi.check()

    def close(self):
        self.check()

    @contextlib.contextmanager
    def no_sync(self):
        """Gradient accumulation: skip communication inside the context; the
        next backward outside it reduces the accumulated gradients."""
        old = self._sync_enabled
        self._sync_enabled = False
        try:
            yield
        finally:
            self._sync_enabled = old


def _native_reducer_available() -> bool:
    try:
        from dmlab import _C
    except ImportError:
        return False
    return hasattr(_C, "Reducer")


DDP = DistributedDataParallel
