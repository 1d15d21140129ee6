"""Autograd operators over the HIP kernels (host side stays Python, as north_star asks): the core every operator family
shares -- every process-wide switch and mutable global (wherever its reader lives), the weight-gradient side stream, the
gradient-buffer contract (_grad_buf, _side_ok, GRAD_SINK), the step-level weight packing, the deferred weight-gradient
queues, conv_c64 / wgrad_c64, the helpers more than one family uses -- and the 64-channel body.

Layout contract: feature maps are logical (B, C, H, W) tensors with channels_last strides, i.e.
physically NHWC, C a multiple of 64; RGB tensors (C == 3) are plain contiguous NCHW.  Every
operator returns tensors in that contract, so a network never converts layouts internally.

Access rule: a family module does `from . import hip, ops` and reaches everything in the core as ops.NAME AT CALL TIME.  It
never does `from .ops import NAME` and never copies a core global into a name of its own: bench.py and the tools replace
ops.conv_c64 / ops.wgrad_c64 and flip ops.WGRAD_SIDE_STREAM while a step runs, the tests flip ops.REFL_GEO, ops.FUSED_GROUPS,
ops.GATE_HEADS and ops.GRAD_SINK, and a name bound at import time would silently escape all of these
(tests/test_ops_layout_cpu.py, tests/test_ops_patch_gpu.py).  This module ends with the imports that re-export every family's
public operators and constants: callers say ops.conv_chain, ops.lam, ops.l1_loss whatever module holds them.

Operators (ops.py unless a module is named)
  conv3x3        default_conv forward/backward incl. fused residual / scalar scale / PixelShuffle store
                 (ref: advanced/common.py:5-8, :20-45)
  res_block      conv-ReLU-conv (+gate) + skip as ONE autograd node: RCAB, QRCAB('standard'), ResBlock,
                 ParamResBlock (ref: advanced/architectures.py:48-71, advanced/common.py:48-72,
                 attention_manipulators/architectures.py:145-180, :332-356)
  meta_gate      ParaCALayer FC stack -> per-(b,c) gate (ref: attention_manipulators/q_layer.py:4-43)
  gated_group    a whole ResidualGroup / QResidualGroup as ONE node (GATE / DOT conv hooks; its weight gradients and gate
                 parameter gradients go out in batches while launches are small: WgradQueue)
  qca_gate       the metadata-mixing QCALayer styles' FC stacks (ref: attention_manipulators/architectures.py:105-127)
  ops_chain.py:  conv_chain / nchw_to_nhwc_pad / pad_param      SRMD (ref: advanced/architectures.py:380-425)
                 frozen_features / FrozenChain    the perceptual loss's VGG19 feature extractor: frozen, once-packed convs,
                 max-pools, input-gradient-only backward (ref: feature_extractors/VGGNets.py:118-131, sr_tools/loss_functions.py:6-22)
  ops_sparnet.py:  refl_conv / batch_norm_act / nearest_up / spar_combine / group_norm / pixel_norm / prelu / shuffle_rgb ...
  ops_sftmd.py:  sft_layer / sft_apply / sftmd_forward          SFTMD (ref: SFTMD_variants/architectures.py:8-176)
  ops_attention.py:  ca_layer / gate_mul / pa_layer ...         stand-alone CALayer / x*gate (ref: advanced/architectures.py:13-32)
                 lam / csam / conv3x3_stack / stack_maps        HAN (ref: advanced/HAN_blocks.py, advanced/architectures.py:314-377)
                 soca / nonlocal_block / nonlocal_attention     SAN (ref: advanced/SAN_blocks.py, advanced/mpncov.py)
                 pixel_shuffle  nn.PixelShuffle on channels-last maps wider than 64 channels (64-wide: fused into the conv's store)
  ops_losses.py:  l1_loss (ref: SISR/models/__init__.py:268) / mse_loss (ref: basic/handlers.py:14) / ssim_mean / ms_ssim_mean / spectral_l1 / degrade_valid
  convs.py:      conv_y2f / conv_f2y / conv_kxk / conv_1x1      SRCNN, VDSR, IKC: K x K convs, the Y-channel ends, pointwise
                 layers (ref: basic/architectures.py:6-77)
  pool.py:       map_mean
  ops_dense.py:  dense_block / dense_skip / dense_conv          RRDBNet: Residual Dense Blocks in place in a 192-channel stack
"""
import functools
import os

import torch
from torch.autograd import Function

from . import hip

CL = torch.channels_last


# ----------------------------------------------------------------------------- side stream for weight gradients
# In a block's backward the weight-gradient kernels (wgrad2, wgrad1) do not feed the data-gradient chain
# (dgrad2 -> dgrad1 -> previous block), so they are issued on a second HIP stream: the ramp-up and tail of
# each ~170 us MFMA launch is then filled by workgroups of the other queue.  The main stream re-joins the side
# stream once, at the end of the backward pass (autograd engine callback), before anything reads the grads.
# (Measured +5 % at 16 tiles per GPU when introduced; neutral at 32 with the current kernels -- see DESIGN.md §3.)
WGRAD_SIDE_STREAM = os.environ.get("SISR_WGRAD_SIDE_STREAM", "1") != "0"
IN_BACKWARD = False  # set while a conv operator's backward runs (bench.py times forward launches only)
_side_streams = {}
_join_pending = set()


def _in_backward(backward):
    """Decorator of a node's backward (under @staticmethod): IN_BACKWARD is True while it runs and False afterwards, whatever
    it was before and however the backward ends."""
    @functools.wraps(backward)
    def wrapped(*args):
        global IN_BACKWARD
        IN_BACKWARD = True
        try:
            return backward(*args)
        finally:
            IN_BACKWARD = False
    return wrapped


def side_stream(device, create=True):
    s = _side_streams.get(device.index)
    if s is None and create:
        s = torch.cuda.Stream(device=device)
        _side_streams[device.index] = s
    return s


def _join_side(device):
    _join_pending.discard(device.index)
    s = _side_streams.get(device.index)
    if s is not None:
        torch.cuda.current_stream(device).wait_stream(s)


def _join_side_now(device):
    """Mid-pass join, for a gradient that autograd is about to add to one the side stream may still be writing: the stream
    that drives the pass waits for what this pass has issued there (nothing, and no wait, when it has issued nothing; the
    end-of-pass join stays queued)."""
    if device.index in _join_pending:
        s = _side_streams.get(device.index)
        if s is not None:
            torch.cuda.current_stream(device).wait_stream(s)


def _side_launch(device, fn, tensors, side=True):
    """Run fn() on the side stream once an event recorded on the main stream now has passed, and keep the caching allocator
    from recycling `tensors` before that stream is done with them; side False (the node's _side_ok answer): call fn() in place."""
    if not side:
        return fn()
    ev = torch.cuda.Event()
    ev.record()
    stream = side_stream(device)
    with torch.cuda.stream(stream):
        stream.wait_event(ev)
        fn()
        for t in tensors:
            if t is not None:
                t.record_stream(stream)
    if device.index not in _join_pending:
        _join_pending.add(device.index)
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _join_side(device))


def _cl(x):
    return x if x.is_contiguous(memory_format=CL) else x.contiguous(memory_format=CL)


def _empty_cl(B, C, H, W, device):
    return torch.empty((B, C, H, W), device=device, dtype=torch.float32, memory_format=CL)


# Data-parallel runs register, per conv weight, the slice of the all-reduce bucket its gradient belongs to
# (parallel.GradReducer): the weight-gradient kernels then write straight into the bucket and the reducer has
# nothing to copy.  Keyed by the parameter's data pointer; empty in single-process runs.
GRAD_SINK = {}

# A backward pass (one autograd graph task) can produce several gradients of one tensor: a weight applied twice.  A leaf's
# .grad stays None until ALL of its contributions have arrived, so `w.grad is None` alone does not say that nobody has been
# promised w's sink, nor that no side-stream launch is still writing a gradient of w.  Two sets of data pointers tell the
# second contribution apart; both are emptied whenever the graph task changes (a pass that died mid-way leaves nothing
# behind).  Host-side only: an ordinary step gains no launch and no synchronisation.
# Limits: the pass is told apart by torch._C._current_graph_task_id(), a private torch call (torch.utils.checkpoint uses
# it too); a NESTED graph task (a reentrant backward, activation checkpointing) empties the sets, so a weight applied once
# before and once after such a nested pass would be handed its sink twice.  Nothing in this package nests passes.
_PASS_ID = -1
_PASS_BUFS = set()    # tensors _grad_buf has handed a gradient buffer out for in this pass
_PASS_SIDE = set()    # weights _side_ok has been asked about in this pass
_PASS_SHARED = set()  # tensors with a second gradient in this pass: never queued by deferred_wgrads()


def _pass_id():
    """The running autograd graph task (-1 outside a backward pass: a backward called by hand accumulates nothing, and
    nothing is recorded); a node with many gradients asks once and hands the answer to _grad_buf."""
    global _PASS_ID
    gid = torch._C._current_graph_task_id()
    if gid != _PASS_ID:
        _PASS_ID = gid
        _PASS_BUFS.clear()
        _PASS_SIDE.clear()
        _PASS_SHARED.clear()
    return gid


def _grad_buf(w, gid=None):
    """The buffer a weight-gradient kernel writes the gradient of `w` into.  Contract (tests/test_autograd_contract_gpu.py):
      * first, or only, gradient of `w` in this backward pass, no .grad yet, a sink registered: a fresh alias of the sink
        (the optimiser's arena slice / the reducer's bucket) -- autograd adopts a gradient it holds the only reference to,
        so the kernel's output IS .grad and nothing is copied;
      * a pre-existing .grad (zero_grad(set_to_none=False), micro-batch accumulation): a private buffer -- autograd adds it
        to .grad, which may itself be the sink view;
      * a further gradient of the same `w` in one pass (a weight applied twice): a private buffer as well -- the sink holds
        the first contribution until autograd has added the two -- handed out only after the side stream has been joined
        and every deferred queue flushed, either of which may still hold the launch of the first one; the launch that fills
        this buffer is never queued itself (wgrad_c64, _ReflConv).  The sum of the two ends in the sink (_sum_into_sink).
    gid: _pass_id(), from a node that asked already."""
    key = w.data_ptr()
    gid = gid if gid is not None else _pass_id()
    # a sink belongs to a leaf parameter.  A non-leaf weight -- the zero-padded copy a ChannelPadded network makes of a
    # parameter every forward -- is a temporary: its address may be the one a parameter of a handler long gone had when it
    # registered its sink, and its gradient must reach autograd (the crop), not that handler's arena
    sink = GRAD_SINK.get(key) if w.is_leaf else None
    if sink is not None and (sink.shape != w.shape or w.grad is not None):
        sink = None
    if gid >= 0:
        if key in _PASS_BUFS:
            if sink is not None and key not in _PASS_SHARED:  # (.grad is still None: the first contribution went to the sink)
                _sum_into_sink(w, sink, gid)
            _PASS_SHARED.add(key)
            _join_side_now(w.device)
            _flush_deferred()
            return torch.empty_like(w)
        _PASS_BUFS.add(key)
    if sink is not None:
        return sink.detach()  # a fresh alias: autograd adopts a gradient it holds the only reference to
    return torch.empty_like(w)


def _sum_into_sink(w, sink, gid):
    """A leaf with two gradients in one pass, the first of them in its sink: the engine adds the two into a tensor of its own
    (it adds in place only into a tensor whose storage nobody else holds, and the sink's alias shares the arena's), so .grad
    would end OUTSIDE the sink and the optimiser / reducer would copy it in later.  A one-shot hook on the leaf moves the sum
    into the sink as soon as the engine has it and hands autograd the alias instead: .grad ends in the sink, as it does for a
    weight applied once.  Nothing is done in a later pass (one that died before the hook ran leaves it behind) or into a
    .grad that exists."""
    def hook(g):
        handle.remove()
        if _PASS_ID != gid or torch._C._current_graph_task_id() != gid or w.grad is not None or g.data_ptr() == sink.data_ptr():
            return None
        sink.copy_(g)
        return sink.detach()
    handle = w.register_hook(hook)


def _grad_buf_or(p, n, device, gid=None):
    """_grad_buf for an optional small parameter (bias): a plain [n] buffer when there is none."""
    return _grad_buf(p, gid) if p is not None else torch.empty(n, device=device)


def _wb_grad_bufs(weight, bias, want_dw, want_db):
    """Buffers of a node whose ONE launch makes the weight's and the bias's gradient, when it is made at all
    -> (the buffer the kernel writes the weight gradient into: _grad_buf(weight), or scratch for a frozen weight, whose
    gradient is dropped; the bias gradient's buffer or None; what the node returns as dw).  _grad_buf hears of the weight first."""
    dwb = _grad_buf(weight) if want_dw else torch.empty_like(weight)
    return dwb, (_grad_buf(bias) if want_db else None), (dwb if want_dw else None)


def _side_ok(*weights, pixels=None):
    """pixels (B * H * W of the launches): inside a deferred_wgrads() block small weight gradients are queued for batched
    launches on the main stream instead (a queue flushed from the side stream would read operands the allocator only tracks
    on the main stream).
    Weight gradients may be produced on the side stream (which re-joins the main stream only at the end of the
    backward pass) iff autograd will merely ADOPT them: with an existing .grad AccumulateGrad would run
    `p.grad += dw` on the main stream before the side-stream kernel has written dw.  The same holds for a weight that is not a
    leaf (one computed from parameters, e.g. SRMD's transposed-conv tail): its gradient is consumed by further backward nodes
    on the main stream at once.  And the same holds for a weight applied twice (named twice here, or one an earlier node of
    this pass has produced a gradient of): autograd adds the two contributions on the main stream as soon as the second node
    returns, so the second goes out on the main stream, behind whatever the side stream still holds of the first.
    A node asks BEFORE it requests its buffers from _grad_buf (which records them as produced): asked afterwards, every
    weight would look like a second contribution and the node would lose the side stream on every ordinary pass
    (tests/test_autograd_contract_cpu.py pins the order on a stand-in node)."""
    if _pass_id() >= 0:
        keys = [w.data_ptr() for w in weights]
        shared = len(set(keys)) < len(keys) or not (_PASS_SIDE.isdisjoint(keys) and _PASS_BUFS.isdisjoint(keys))
        _PASS_SIDE.update(keys)
        if shared:
            _join_side_now(weights[0].device)
            return False
    if not (WGRAD_SIDE_STREAM and torch.is_grad_enabled() is False and all(w.is_leaf and w.grad is None for w in weights)):
        return False
    if _DEFERRED is not None and pixels is not None and PRECISION == "fp32" and pixels <= BATCH_WGRAD_MAX_PIXELS:
        return False
    # under hipGraph capture the fork / join would become graph edges (measured slower than one stream): one stream there
    return not torch.cuda.is_current_stream_capturing()


_gate_ws_cache = {}


def _gate_ws(B, device):
    """Scratch of sisr_ca_gate_bwd ([B][80] floats), one per (device, batch): a named, persistent tensor -- a
    temporary built inside the call expression is released before the launch and the very next allocation (the
    lazily created gate counter, once) can be handed the same block."""
    key = (device.index, B)
    t = _gate_ws_cache.get(key)
    if t is None:
        t = torch.empty((B, 80), device=device, dtype=torch.float32)
        _gate_ws_cache[key] = t
    return t


def _vec(B, C, device):
    return torch.empty((B, C), device=device, dtype=torch.float32)


# ----------------------------------------------------------------------------- raw launches (no autograd)
# Arithmetic of the 64-channel-chunk convolutions (forward, input gradient, weight gradient):
#   "fp32"  v_mfma_f32_32x32x2_f32, exact fp32 -- the reference's arithmetic, the default
#   "bf16"  v_mfma_f32_32x32x16_bf16: both operands rounded to bf16 (RNE) on their way into LDS, fp32 accumulate,
#           fp32 feature maps / gradients / optimiser state in HBM (BASELINE config "HAN x4 bf16 ... MFMA")
#   "bf16x3" forward and input-gradient convs with every fp32 operand split exactly into three bf16 numbers and the six
#           significant products on the bf16 matrix cores (fp32-class error, 6/16 of the fp32 MFMA's cycles), weight
#           gradients likewise.  Opt-in, never the headline
# Process-wide; packed weights are rebuilt every step, so switching between steps is safe.
PRECISION = os.environ.get("SISR_PRECISION", "fp32")
X3_WGRAD = os.environ.get("SISR_X3_WGRAD", "1") != "0"  # bf16x3 mode: weight gradients split too (0: exact fp32 kernel)
FUSED_GROUPS = os.environ.get("SISR_FUSED_GROUPS", "1") != "0"  # group-level autograd node for CA block stacks


def set_precision(name):
    global PRECISION
    if name not in ("fp32", "bf16", "bf16x3"):
        raise ValueError(f"precision must be 'fp32', 'bf16' or 'bf16x3', got {name!r}")
    PRECISION = name


def _wptr(packed):
    return hip.ptr_bf16(packed) if packed.dtype == torch.bfloat16 else hip.ptr(packed)


# Step-level packing: BaseModel.train_step / run_eval call pack_all(net) once, which repacks EVERY conv weight of the
# network with one launch into persistent buffers and publishes them here; pack_pair / pack_weight then find their
# weight (by object identity) and launch nothing.  The entries are dropped as soon as the optimiser has moved the
# weights (invalidate_packs), so a stale packing can never be used; code that calls a network outside the handlers
# simply packs per conv as before.
_STEP_PACKS = {}


_PACK_WINOGRAD = 0x100  # PackJob.r flag (conv3x3_mfma.hip: SISR_PACK_WINOGRAD)
WINOGRAD_FLOATS = 16 * 64 * 64  # transformed 64 x 64 weight block, behind the whole direct packing: one per pair of chunks
SELECT_WINOGRAD, SELECT_WINOGRAD_FORCE = 11, 12  # `select` codes: the packed weight carries the transform (auto / forced)
SELECT_WINOGRAD_PREDICATED = 14  # ... forced, with the predicated epilogue on every tile (tests of the full-tile epilogue)


class _PackPlan:
    def __init__(self, weights, device):
        import numpy as np
        self.precision = PRECISION
        self.items = [(w, int(r)) for w, r in weights]
        self.ptrs = [w.data_ptr() for w, _ in self.items]
        planes = 3 if PRECISION == "bf16x3" else 1
        # a weight whose channel counts are not multiples of 64 (SPARNet) is packed as its zero-padded twin, same launch
        padded = [(_pad64(w.shape[0]), _pad64(w.shape[1])) for w, _ in self.items]
        numel = [co * ci * 9 for co, ci in padded]
        # fp32 64 -> 64 weights, and the 64 -> 64 r^2 weights of a conv with a fused PixelShuffle(r), also get their Winograd
        # F(2x2,3x3) transform right behind the direct packing (both orders, one block per pair of 64-channel chunks);
        # conv_c64 sees it in the slice length and lets the library use the Winograd kernel where it pays
        wino = [PRECISION == "fp32" and p == (64 * r * r, 64) == tuple(w.shape[:2]) for (w, r), p in zip(self.items, padded)]
        pairs = [(co // 64) * (ci // 64) for co, ci in padded]
        extra = [pairs[k] * WINOGRAD_FLOATS if wino[k] else 0 for k in range(len(wino))]
        total = planes * sum(numel) + sum(extra)
        dt = torch.float32 if PRECISION == "fp32" else torch.bfloat16
        self.fwd = torch.empty(total, device=device, dtype=dt)
        self.dgrad = torch.empty(total, device=device, dtype=dt)
        esz = self.fwd.element_size()
        jobs = np.zeros(len(self.items), dtype=[("w", "<u8"), ("pf", "<u8"), ("pd", "<u8"), ("cout", "<i4"),
                                                ("cin", "<i4"), ("r", "<i4"), ("first", "<i4"), ("co_real", "<i4"),
                                                ("ci_real", "<i4")])
        assert jobs.dtype.itemsize == hip.lib().sisr_pack_job_bytes()
        off = blocks = 0
        self.slices = []
        for k, (w, r) in enumerate(self.items):
            n = planes * numel[k] + extra[k]
            real = (w.shape[0], w.shape[1]) if padded[k] != (w.shape[0], w.shape[1]) else (0, 0)
            jobs[k] = (w.data_ptr(), self.fwd.data_ptr() + off * esz, self.dgrad.data_ptr() + off * esz, padded[k][0],
                       padded[k][1], r | (_PACK_WINOGRAD if wino[k] else 0), blocks, real[0], real[1])
            self.slices.append((self.fwd[off:off + n], self.dgrad[off:off + n]))
            off += n
            blocks += (numel[k] + 255) // 256 + (16 * pairs[k] if wino[k] else 0)  # + one thread per (ci, co) for the transform
        self.blocks = blocks
        self.jobs = torch.from_numpy(jobs.view(np.uint8)).to(device)

    def valid(self):
        return self.precision == PRECISION and all(w.data_ptr() == p for (w, _), p in zip(self.items, self.ptrs))

    def run(self):
        hip.check(hip.lib().sisr_pack_conv3x3_many(self.jobs.data_ptr(), len(self.items), self.blocks,
                                                   {"fp32": 0, "bf16": 1, "bf16x3": 2}[PRECISION], hip.stream()),
                  "sisr_pack_conv3x3_many")
        for (w, r), (pf, pd) in zip(self.items, self.slices):
            _STEP_PACKS[id(w)] = (w, r, PRECISION, pf, pd)


_SFT_STEP = {}  # id(mul_conv1.weight) -> (that weight, WA, bA, WB, bB): merged SFT weights composed for this step


class _SftComposePlan:
    """Merged weights of every StandardSft of a network, composed in one launch (sisr_sft_compose_many) into persistent
    buffers; their MFMA packings then ride along in the network's one-launch weight packing."""

    def __init__(self, mods, device):
        import numpy as np
        self.mods = mods
        self.merged = [(torch.empty((64, 128, 3, 3), device=device), torch.empty(64, device=device),
                        torch.empty((128, 64, 3, 3), device=device), torch.empty(128, device=device)) for _ in mods]
        rec = np.zeros(len(mods), dtype=[("p", "<u8", (12,)), ("M", "<i4"), ("split", "<i4")])
        assert rec.dtype.itemsize == hip.lib().sisr_sft_compose_record_bytes()
        self.ptrs = []
        for k, m in enumerate(mods):
            ps = [t.data_ptr() for t in m.params()] + [t.data_ptr() for t in self.merged[k]]
            rec[k] = (ps, m.mul_conv1.weight.shape[1] - 64, 0)
            self.ptrs.append(ps[:8])
        self.table = torch.from_numpy(rec.view(np.uint8)).to(device)

    def valid(self):
        return all(all(t.data_ptr() == q and t.is_contiguous() for t, q in zip(m.params(), ps))
                   for m, ps in zip(self.mods, self.ptrs))

    def run(self):
        hip.check(hip.lib().sisr_sft_compose_many(self.table.data_ptr(), len(self.mods), hip.stream()), "sisr_sft_compose_many")
        for m, mg in zip(self.mods, self.merged):
            w = m.mul_conv1.weight
            _SFT_STEP[id(w)] = (w, *mg)

    def weights(self):
        out = []
        for WA, _, WB, _ in self.merged:
            out += [(WA, 1), (WB, 1)]
        return out


def _sft_plan(net):
    mods = [m for m in net.modules() if type(m).__name__ == "StandardSft" and m.mul_conv1.weight.is_cuda]
    if not mods or PRECISION != "fp32" or not all(t.is_contiguous() for m in mods for t in m.params()):
        return None
    plan = getattr(net, "_sisr_sft_plan", None)
    if plan is None or not plan.valid():
        plan = _SftComposePlan(mods, mods[0].mul_conv1.weight.device)
        net._sisr_sft_plan = plan
        net._sisr_pack_plan = None  # the merged buffers are new tensors: rebuild the packing plan around them
    return plan


def pack_all(net, weights_fn):
    """Repack every 64-multiple 3x3 conv weight of `net` in one launch; weights_fn(net) -> [(weight, shuffle)].  SFT layers:
    their merged weights are composed first (one launch for all of them) and packed in the same launch as the rest."""
    sft = _sft_plan(net)
    if sft is not None:
        sft.run()
    plan = getattr(net, "_sisr_pack_plan", None)
    if plan is None or not plan.valid():
        ws = [(w, r) for w, r in weights_fn(net) if w.is_cuda and w.is_contiguous()]
        if sft is not None:
            ws += sft.weights()
        if not ws:
            return
        plan = _PackPlan(ws, ws[0][0].device)
        net._sisr_pack_plan = plan
    plan.run()


def invalidate_packs():
    _STEP_PACKS.clear()
    _SFT_STEP.clear()


def _step_pack(w, shuffle):
    e = _STEP_PACKS.get(id(w))
    if e is not None and e[0] is w and e[1] == shuffle and e[2] == PRECISION:
        return e[3], e[4]
    return None


def pack_weight(w, mode, shuffle=1):
    """OIHW fp32 weight -> B-fragment order of the MFMA conv ('fwd') or of its input gradient ('dgrad')."""
    hit = _step_pack(w, shuffle)
    if hit is not None:
        return hit[0] if mode == "fwd" else hit[1]
    if PRECISION != "fp32":
        pf, pd = pack_pair(w, shuffle)
        return pf if mode == "fwd" else pd
    cout, cin = w.shape[0], w.shape[1]
    packed = torch.empty(cout * cin * 9, device=w.device, dtype=torch.float32)
    rr = shuffle * shuffle
    if mode == "fwd":
        on, oq = (rr, 1) if shuffle > 1 else (1, 64)
        rc = hip.lib().sisr_pack_conv3x3(hip.ptr(w), hip.ptr(packed), cout, cin, cin * 9, 9, 0, on, oq, 1, 64,
                                         hip.stream())
    else:
        in_, iq = (rr, 1) if shuffle > 1 else (1, 64)
        rc = hip.lib().sisr_pack_conv3x3(hip.ptr(w), hip.ptr(packed), cin, cout, 9, cin * 9, 1, 1, 64, in_, iq,
                                         hip.stream())
    hip.check(rc, "sisr_pack_conv3x3")
    return packed


def pack_pair(w, shuffle=1):
    """(forward packing, input-gradient packing) of one weight, one launch."""
    hit = _step_pack(w, shuffle)
    if hit is not None:
        return hit
    cout, cin = w.shape[0], w.shape[1]
    if PRECISION == "bf16x3":
        buf = torch.empty(2, 3 * cout * cin * 9, device=w.device, dtype=torch.bfloat16)
        hip.check(hip.lib().sisr_pack_conv3x3_x3_both(hip.ptr(w), hip.ptr_bf16(buf[0]), hip.ptr_bf16(buf[1]), cout, cin,
                                                      shuffle, hip.stream()), "sisr_pack_conv3x3_x3_both")
        return buf[0], buf[1]
    if PRECISION == "bf16":
        buf = torch.empty(2, cout * cin * 9, device=w.device, dtype=torch.bfloat16)
        hip.check(hip.lib().sisr_pack_conv3x3_bf16_both(hip.ptr(w), hip.ptr_bf16(buf[0]), hip.ptr_bf16(buf[1]), cout,
                                                        cin, shuffle, hip.stream()), "sisr_pack_conv3x3_bf16_both")
        return buf[0], buf[1]
    buf = torch.empty(2, cout * cin * 9, device=w.device, dtype=torch.float32)
    hip.check(hip.lib().sisr_pack_conv3x3_both(hip.ptr(w), hip.ptr(buf[0]), hip.ptr(buf[1]), cout, cin, shuffle,
                                               hip.stream()), "sisr_pack_conv3x3_both")
    return buf[0], buf[1]


def conv_c64(x, xview, packed, bias, bias_nq, y, yview, B, H, W, cin, cout, res=None, mask=None, in_scale=None,
             in_shift=None, out_scale=None, alpha=1.0, relu=False, gap=None, gate_add=None, gate_out=None, dot=None,
             select=0, ca_head=None):
    """ca_head: an fp32 gate head (hip.CaTail with head = 1): the channel-attention gate, or the per-sample part of its
    backward, computed by this conv from the partial sums it consumes."""
    L = hip.lib()
    # the packing decides: a weight packed under one mode runs under it (three bf16 planes = the bf16x3 split)
    if packed.dtype != torch.bfloat16:
        import ctypes
        if select == 0 and packed.numel() == cin * cout * 9 + (cin // 64) * (cout // 64) * WINOGRAD_FLOATS:
            select = SELECT_WINOGRAD
        rc = L.sisr_conv3x3_c64(hip.ptr(x), xview, _wptr(packed), hip.ptr(bias), bias_nq[0], bias_nq[1], hip.ptr(y), yview,
                                hip.ptr(res), hip.ptr(mask), hip.ptr(in_scale), hip.ptr(in_shift), hip.ptr(out_scale),
                                float(alpha), int(relu), hip.ptr(gap), hip.ptr(gate_add), hip.ptr(gate_out), hip.ptr(dot), B,
                                H, W, cin, cout, ctypes.addressof(ca_head) if ca_head is not None else None, int(select),
                                hip.stream())
        hip.check(rc, "sisr_conv3x3_c64")
        return
    if ca_head is not None:
        raise RuntimeError("gate heads exist on the fp32 conv kernels only")
    if packed.numel() == 3 * cin * cout * 9:
        fn, name = L.sisr_conv3x3_c64_x3, "sisr_conv3x3_c64_x3"
    else:
        fn, name = L.sisr_conv3x3_c64_bf16, "sisr_conv3x3_c64_bf16"
    rc = fn(hip.ptr(x), xview, _wptr(packed), hip.ptr(bias), bias_nq[0], bias_nq[1], hip.ptr(y), yview, hip.ptr(res),
            hip.ptr(mask), hip.ptr(in_scale), hip.ptr(in_shift), hip.ptr(out_scale), float(alpha), int(relu),
            hip.ptr(gap), hip.ptr(gate_add), hip.ptr(gate_out), hip.ptr(dot), B, H, W, cin, cout, int(select), hip.stream())
    hip.check(rc, name)


# bf16 STORAGE (on top of PRECISION == "bf16", BASELINE config 5): the maps a residual group keeps for itself and for its
# backward pass -- t1 = ReLU(conv1), t2 = conv2, the gated skips u_k -- live in HBM as bf16 (rounded once, where they are
# written; read back without conversion as MFMA operands), which halves what the group's HBM-bound kernels move for them.
# Group inputs / outputs, gradient maps, gates, partial sums, weights' master copies and the optimiser stay fp32.
#   "0"    fp32 maps (the default)      "act"  the group's activations as above
#   "all"  ... and the gradient maps the group's backward pass hands from launch to launch (dU_k, dt1): rounded once where
#          they are written, after the ReLU mask / the skip's gradient have been applied in fp32; the partial sums of the gate
#          gradients and the bias gradients are taken from fp32 values, the group's input gradient leaves it in fp32
BF16_STORAGE = os.environ.get("SISR_BF16_STORAGE", "0")


def set_storage(name):
    """Storage format of the maps a residual group keeps, in the bf16 operand mode: "0" (fp32), "act" (bf16 activations) or
    "all" (bf16 activations and gradient maps)."""
    global BF16_STORAGE
    if name not in ("0", "act", "all"):
        raise ValueError(f"storage must be '0', 'act' or 'all', got {name!r}")
    BF16_STORAGE = name


def _empty_cl16(B, C, H, W, device):
    return torch.empty((B, C, H, W), device=device, dtype=torch.bfloat16, memory_format=CL)


def to_bf16_map(x):
    """fp32 channels-last map -> bf16 channels-last map (round to nearest even), one launch."""
    y = _empty_cl16(*x.shape, x.device)
    hip.check(hip.lib().sisr_f32_to_bf16(hip.ptr(x), hip.ptr_any(y), x.numel(), hip.stream()), "sisr_f32_to_bf16")
    return y


def conv_c64s(x, packed, bias, y, B, H, W, storage, res=None, mask=None, in_scale=None, in_shift=None, alpha=1.0, relu=False,
              gap=None, gate_add=None, gate_out=None, dot=None):
    """64 -> 64 conv of the bf16 operand mode with bf16-stored maps (include/sisr_hip.h: sisr_conv3x3_c64_bf16s storage bits)."""
    if packed.dtype != torch.bfloat16 or packed.numel() != 64 * 64 * 9:
        raise RuntimeError("bf16 storage needs a weight packed in the bf16 operand mode (64 -> 64)")
    v = hip.view_plain(H, W, 64)
    rc = hip.lib().sisr_conv3x3_c64_bf16s(hip.ptr_any(x), v, _wptr(packed), hip.ptr(bias), 1, 64, hip.ptr_any(y), v,
                                          hip.ptr_any(res), hip.ptr_any(mask), hip.ptr(in_scale), hip.ptr(in_shift), float(alpha),
                                          int(relu), hip.ptr(gap), hip.ptr_any(gate_add), hip.ptr_any(gate_out), hip.ptr_any(dot),
                                          B, H, W, int(storage), hip.stream())
    hip.check(rc, "sisr_conv3x3_c64_bf16s")


_DEFERRED = None  # {(B, H, W, device index): WgradQueue} while a deferred_wgrads() block is open
_DEFERRED_STREAM = None  # the stream the block was opened on: launches issued from another stream are not queued


class deferred_wgrads:
    """While open (around ONE backward pass), plain 64 -> 64 weight gradients of small launches are queued and go out eight at
    a time (WgradQueue), the rest when the block closes.  Only sound when nothing reads a parameter gradient before the block
    closes: the handlers open it when no reducer hook can fire (single process, or hipGraph capture / replay where the
    buckets are reduced at the join).  A launch is queued only when autograd will merely ADOPT its result, and then writes,
    late, into the tensors autograd has adopted as .grad.  Two queues, two rules.  wgrad_c64 (the 64 -> 64 convs): the WEIGHT
    is a trainable leaf whose .grad is None; the conv's bias gradient rides in the same launch -- a frozen bias's lands in a
    buffer nobody adopts (its storage is kept until the flush), a frozen weight's launch, made for a trainable bias, is not
    queued at all.  _ReflConv (SPARNet's convs): weight AND bias are trainable leaves without a .grad, else the launch goes
    out directly.  With a .grad that exists already (zero_grad(set_to_none=False), micro-batch accumulation) nothing is
    queued and autograd adds the result as usual.
    (tests/test_autograd_contract_gpu.py pins all of this: frozen subsets, kept and shared gradients, inside the block and out.)

    Two guards keep a queued gradient from ever being read unwritten:
      * the block flushes on EVERY exit, exceptional ones included: a queue entry keeps the storages of its output buffers
        alive (not the tensors -- see WgradQueue.add), so the late launches are memory-safe even if the backward pass died
        before autograd adopted them, and every .grad that was adopted holds its gradient when the block has closed;
      * a weight is queued at most once per block: a second weight gradient of the same parameter (a conv weight used twice
        in one backward) first flushes every queue -- autograd sums the two results as soon as the second arrives, on this
        stream -- and is launched directly, into a buffer of its own.  _grad_buf does both when it is asked for a second
        buffer of one tensor in a pass, whatever the two launches look like (one of them may be ineligible for the queue:
        another alpha, a shuffle); the _DEFERRED_OWNERS check below covers weight gradients that bypass _grad_buf."""

    def __init__(self, enabled=True):
        self.enabled = enabled and BATCH_WGRAD

    def __enter__(self):
        global _DEFERRED, _DEFERRED_STREAM, _DEFERRED_OWNERS
        if self.enabled:
            _DEFERRED, _DEFERRED_STREAM = {}, torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
            _DEFERRED_OWNERS = set()
        return self

    def __exit__(self, *exc):
        global _DEFERRED, _DEFERRED_OWNERS
        queues, _DEFERRED, _DEFERRED_OWNERS = _DEFERRED, None, None
        if queues:
            for q in queues.values():
                try:
                    q.flush()
                except Exception:
                    if exc[0] is None:
                        raise  # on an exceptional exit the first error is the one to report
        return False


_DEFERRED_OWNERS = None  # ids of the weights with a queued gradient in the open deferred_wgrads() block


def _flush_deferred():
    if _DEFERRED:
        for q in _DEFERRED.values():
            q.flush()


def wgrad_c64(x, xview, dy, dyview, dw, db, B, H, W, cin, cout, alpha=1.0, dy_scale=None, dy_shift=None, shuffle=1,
              active_units=0, owner=None, storage=0):
    """active_units (fp32 kernel): bit mask of the 32 x 32-channel blocks of the gradient to compute (0 = all).
    owner: the weight Parameter -- with it, inside a deferred_wgrads() block, an eligible launch is queued instead."""
    # (a non-leaf owner -- a ChannelPadded network's padded weight -- is never queued: autograd crops its gradient as soon as
    # this node returns, long before the block's flush would have written it)
    if (_DEFERRED is not None and hip.stream() == _DEFERRED_STREAM and owner is not None and owner.requires_grad and
            owner.is_leaf and owner.grad is None and owner.data_ptr() not in _PASS_SHARED and cin == 64 and cout == 64 and shuffle == 1 and
            alpha == 1.0 and not active_units and WgradQueue.wanted(B, H, W) and xview is hip.view_plain(H, W, 64) and
            dyview is hip.view_plain(H, W, 64)):
        if id(owner) in _DEFERRED_OWNERS:
            _flush_deferred()  # second gradient of one weight in this pass: the first must be written before autograd adds them
        else:
            _DEFERRED_OWNERS.add(id(owner))
            key = (B, H, W, x.device.index)
            q = _DEFERRED.get(key)
            if q is None:
                q = _DEFERRED[key] = WgradQueue(B, H, W, x.device)
            q.add(x, dy, dw, db, dy_scale=dy_scale, dy_shift=dy_shift, hold_outputs=False)
            return
    L = hip.lib()
    fp32 = False
    if PRECISION == "bf16x3" and X3_WGRAD:
        size_fn, fn, name = L.sisr_wgrad3x3_c64_x3_workspace_bytes, L.sisr_wgrad3x3_c64_x3, "sisr_wgrad3x3_c64_x3"
    elif PRECISION == "bf16":
        size_fn, fn, name = L.sisr_wgrad3x3_c64_bf16_workspace_bytes, L.sisr_wgrad3x3_c64_bf16, "sisr_wgrad3x3_c64_bf16"
    else:
        size_fn, fn, name, fp32 = L.sisr_wgrad3x3_c64_workspace_bytes, L.sisr_wgrad3x3_c64, "sisr_wgrad3x3_c64", True
    nbytes = size_fn(B, H, W, cin, cout)
    ws = hip.workspace(x.device, nbytes)
    rr = shuffle * shuffle
    on, oq = (rr, 1) if shuffle > 1 else (1, 64)
    if storage:  # bf16-stored x (1) or x and dY (3): the bf16 operand mode's kernel reading 2-byte elements
        if PRECISION != "bf16":
            raise RuntimeError("bf16-stored maps exist in the bf16 operand mode only")
        fn, name = L.sisr_wgrad3x3_c64_bf16s, "sisr_wgrad3x3_c64_bf16s"
        args = (hip.ptr_any(x), xview, hip.ptr_any(dy), dyview, hip.ptr(dy_scale), hip.ptr(dy_shift), float(alpha), hip.ptr(dw),
                cin * 9, 9, 0, on, oq, 1, 64, hip.ptr(db), on, oq, hip.ptr(ws), nbytes, B, H, W, cin, cout)
        hip.check(fn(*args, int(storage), hip.stream()), name)
        return
    args = (hip.ptr(x), xview, hip.ptr(dy), dyview, hip.ptr(dy_scale), hip.ptr(dy_shift), float(alpha), hip.ptr(dw),
            cin * 9, 9, 0, on, oq, 1, 64, hip.ptr(db), on, oq, hip.ptr(ws), nbytes, B, H, W, cin, cout)
    rc = fn(*args, int(active_units), hip.stream()) if fp32 else fn(*args, hip.stream())
    hip.check(rc, name)


# Weight gradients of one geometry are launched eight at a time while a launch is small (<= BATCH_WGRAD_MAX_PIXELS pixels per
# map: up to 8 tiles of 128 x 128 per GPU -- BASELINE config 4 has 4): see csrc/wgrad3x3_mfma.hip wgrad3x3_c64_batch_kernel.
BATCH_WGRAD = os.environ.get("SISR_BATCH_WGRAD", "1") != "0"
# ... and in the same regime the channel-attention gate (and its backward) is computed by the conv that consumes it (gate
# HEADS, csrc/conv3x3_mfma.hip template HEAD) instead of a 6 us launch of its own between two convs of the serial chain.
GATE_HEADS = os.environ.get("SISR_GATE_HEADS", "1") != "0"
GATE_HEADS_MAX_PIXELS = int(os.environ.get("SISR_GATE_HEADS_MAX_PIXELS", 4 * 128 * 128))  # measured: +2.3 % at 4 tiles, -1 % at 8
# jobs per launch: the library's maximum, 8 (full per-job argument records by value in the launch arguments).  A variant with
# slim records and up to 48 jobs per launch (a whole group's 41 in one) was tried: the argument struct copied per job went to
# scratch memory and the step got 11 % slower; eight also keeps what the jobs read (2 x 8 maps of 16.8 MB) recent.
BATCH_WGRAD_JOBS = int(os.environ.get("SISR_BATCH_WGRAD_JOBS", 8))
BATCH_WGRAD_MAX_PIXELS = int(os.environ.get("SISR_BATCH_WGRAD_MAX_PIXELS", 8 * 128 * 128))


class WgradQueue:
    """64 -> 64 weight gradients of one (B, H, W) queued by a backward pass and launched in batches (flush() before the
    gradients leave the autograd node).  Holds references to every operand until its launch has been issued."""

    def __init__(self, B, H, W, device):
        self.geo, self.device, self.jobs = (B, H, W), device, []
        self.max = min(BATCH_WGRAD_JOBS, hip.lib().sisr_wgrad3x3_c64_batch_max())

    @staticmethod
    def wanted(B, H, W):
        return BATCH_WGRAD and PRECISION == "fp32" and B * H * W <= BATCH_WGRAD_MAX_PIXELS

    def add(self, x, dy, dw, db, dy_scale=None, dy_shift=None, hold_outputs=True):
        """hold_outputs=False: keep only the ADDRESSES of dw / db, and their STORAGES.  A queue that outlives the autograd node
        must not hold references to the gradient tensors the node returns: AccumulateGrad adopts a gradient only if it holds
        the sole reference to the tensor and clones it otherwise -- the clone would be taken before the launch has written it.
        A storage reference does not count there, and it keeps the memory from being recycled before the flush even when
        the backward pass dies before the gradient is adopted."""
        if hold_outputs:
            self.jobs.append((x, dy, dy_scale, dy_shift, dw, db, None))
        else:
            keep = (dw.untyped_storage(), db.untyped_storage() if db is not None else None)
            self.jobs.append((x, dy, dy_scale, dy_shift, hip.ptr(dw), hip.ptr(db), keep))
        if len(self.jobs) == self.max:
            self.flush()

    def flush(self):
        if not self.jobs:
            return
        B, H, W = self.geo
        L, n = hip.lib(), len(self.jobs)
        arr = (hip.WgradJob * n)()
        for k, (x, dy, sc, sh, dw, db, _) in enumerate(self.jobs):
            arr[k].x, arr[k].dy, arr[k].dy_scale, arr[k].dy_shift = hip.ptr(x), hip.ptr(dy), hip.ptr(sc), hip.ptr(sh)
            arr[k].dw, arr[k].dbias = (dw, db) if isinstance(dw, int) else (hip.ptr(dw), hip.ptr(db))
        nbytes = L.sisr_wgrad3x3_c64_batch_workspace_bytes(n, B, H, W)
        ws = hip.workspace(self.device, nbytes)
        v = hip.view_plain(H, W, 64)
        import ctypes
        hip.check(L.sisr_wgrad3x3_c64_batch(ctypes.addressof(arr), n, v, v, hip.ptr(ws), nbytes, B, H, W, hip.stream()),
                  "sisr_wgrad3x3_c64_batch")
        self.jobs = []


class WgradGeoQueue:
    """Weight gradients of SPARNet's ConvLayer convs (any geometry) queued by a backward pass inside a deferred_wgrads() block
    and launched eight per launch, similar sizes together, when the block closes (sisr_wgrad3x3_c64_geo_batch).  Holds the
    operands, and the STORAGES of the outputs (see WgradQueue.add), until the launches have been issued."""
    MAX_JOBS = 256  # flush earlier than the end of the pass beyond this (bounds what the queue keeps alive)

    def __init__(self, device):
        self.device, self.jobs = device, []

    def add(self, x, dy, dw, db, ints, units, work):
        keep = (dw.untyped_storage(), db.untyped_storage() if db is not None else None)
        self.jobs.append((work, x, dy, hip.ptr(dw), hip.ptr(db), ints, units, keep))
        if len(self.jobs) >= self.MAX_JOBS:
            self.flush()

    def flush(self):
        if not self.jobs:
            return
        import ctypes
        L = hip.lib()
        if L.sisr_wgrad_geo_job_bytes() != ctypes.sizeof(hip.WgradGeoJob):
            raise RuntimeError("hip.WgradGeoJob does not match sisr_wgrad_geo_job of the loaded library")
        jobs = sorted(self.jobs, key=lambda j: j[0])  # launches of eight similar sizes
        arr = (hip.WgradGeoJob * len(jobs))()
        for k, (_, x, dy, dw, db, ints, units, _keep) in enumerate(jobs):
            a = arr[k]
            a.x, a.dy, a.dw, a.dbias = hip.ptr(x), hip.ptr(dy), dw, db
            a.B, a.H, a.W, a.cin, a.cout, a.up, a.co_real, a.ci_real = ints
            a.active_units = units
        nbytes = L.sisr_wgrad3x3_c64_geo_batch_workspace_bytes(ctypes.addressof(arr), len(jobs))
        ws = hip.workspace(self.device, nbytes)
        hip.check(L.sisr_wgrad3x3_c64_geo_batch(ctypes.addressof(arr), len(jobs), hip.ptr(ws), nbytes, hip.stream()),
                  "sisr_wgrad3x3_c64_geo_batch")
        self.jobs = []


def gap_parts(H, W):
    return hip.lib().sisr_conv3x3_c64_gap_parts(H, W)


# ----------------------------------------------------------------------------- conv3x3
class _Conv3x3(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, alpha, shuffle):
        cout, cin = weight.shape[0], weight.shape[1]
        B, _, H, W = x.shape
        dev = x.device
        w = weight.contiguous()
        ctx.alpha, ctx.shuffle, ctx.geom = alpha, shuffle, (B, H, W, cin, cout)
        ctx.has_res = residual is not None
        if cin % 64 == 0 and cout % 64 == 0:
            x = _cl(x)
            if ctx.needs_input_grad[0]:
                packed, ctx.packed_dgrad = pack_pair(w, shuffle)
            else:
                packed, ctx.packed_dgrad = pack_weight(w, "fwd", shuffle), None
            if shuffle > 1:
                if cout != 64 * shuffle * shuffle:
                    raise NotImplementedError("fused PixelShuffle needs Cout == 64*r*r")
                y = _empty_cl(B, 64, H * shuffle, W * shuffle, dev)
                yview, bnq = hip.view_shuffle(H, W, shuffle), (shuffle * shuffle, 1)
            else:
                y = _empty_cl(B, cout, H, W, dev)
                yview, bnq = hip.view_plain(H, W, cout), (1, 64)
            res = _cl(residual) if residual is not None else None
            conv_c64(x, hip.view_plain(H, W, cin), packed, bias, bnq, y, yview, B, H, W, cin, cout, res=res,
                     alpha=alpha)
            ctx.kind = "c64"
        elif cin == 3 and cout % 64 == 0:
            if shuffle > 1 or residual is not None or alpha != 1.0:
                raise NotImplementedError("3->64k conv has no fused epilogue")
            x = x.contiguous()
            y = _empty_cl(B, cout, H, W, dev)
            rc = hip.lib().sisr_conv3x3_cin3(hip.ptr(x), hip.ptr(w), 27, 9, 0, hip.ptr(bias), hip.ptr(y),
                                             hip.view_plain(H, W, cout), B, H, W, cout, hip.stream())
            hip.check(rc, "sisr_conv3x3_cin3")
            ctx.kind = "cin3"
        elif cout == 3 and cin % 64 == 0:
            if shuffle > 1 or residual is not None or alpha != 1.0:
                raise NotImplementedError("64k->3 conv has no fused epilogue")
            x = _cl(x)
            y = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
            rc = hip.lib().sisr_conv3x3_cout3(hip.ptr(x), hip.view_plain(H, W, cin), hip.ptr(w), cin * 9, 9, 0,
                                              hip.ptr(bias), hip.ptr(y), B, H, W, cin, hip.stream())
            hip.check(rc, "sisr_conv3x3_cout3")
            ctx.kind = "cout3"
        else:
            raise NotImplementedError(
                f"conv3x3 {cin}->{cout}: the gfx950 kernels cover channel counts that are multiples of 64 and the "
                f"3-channel RGB ends (the reference's in-scope configs all use n_feats = 64 or 256)")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.bias = bias  # the leaf itself: its gradient goes straight into the optimiser's arena when it has a slot there
        return y

    @staticmethod
    @_in_backward
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, H, W, cin, cout = ctx.geom
        dev = x.device
        L = hip.lib()
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dx = dw = db = dres = None
        if ctx.kind == "c64":
            dy = _cl(dy)
            r = ctx.shuffle
            dyview = hip.view_shuffle(H, W, r) if r > 1 else hip.view_plain(H, W, cout)
            if need_x:
                packed = ctx.packed_dgrad if ctx.packed_dgrad is not None else pack_weight(w, "dgrad", r)
                dx = _empty_cl(B, cin, H, W, dev)
                conv_c64(dy, dyview, packed, None, (1, 64), dx, hip.view_plain(H, W, cin), B, H, W, cout, cin,
                         alpha=ctx.alpha)
            if need_w or need_b:
                dw = _grad_buf(w)
                db = _grad_buf(ctx.bias) if ctx.has_bias else None
                wgrad_c64(x, hip.view_plain(H, W, cin), dy, dyview, dw, db, B, H, W, cin, cout, alpha=ctx.alpha,
                          shuffle=r, owner=w)
            if ctx.has_res and need_r:
                dres = dy
        elif ctx.kind == "cin3":
            dy = _cl(dy)
            if need_x:
                dx = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
                rc = L.sisr_conv3x3_cout3(hip.ptr(dy), hip.view_plain(H, W, cout), hip.ptr(w), 9, 27, 1, None,
                                          hip.ptr(dx), B, H, W, cout, hip.stream())
                hip.check(rc, "sisr_conv3x3_cout3(dgrad)")
            if need_w or need_b:
                dw = _grad_buf(w)
                db = _grad_buf(ctx.bias) if ctx.has_bias else None
                nbytes = L.sisr_corr3x3_c3_workspace_bytes(B, H, W, cout)
                ws = hip.workspace(dev, nbytes)
                rc = L.sisr_corr3x3_c3(hip.ptr(x), hip.ptr(dy), hip.view_plain(H, W, cout), 1.0, hip.ptr(dw), 27, 9, 0,
                                       0, hip.ptr(db), hip.ptr(ws), nbytes, B, H, W, cout, hip.stream())
                hip.check(rc, "sisr_corr3x3_c3(head)")
        else:  # cout3
            dy = dy.contiguous()
            if need_x:
                dx = _empty_cl(B, cin, H, W, dev)
                rc = L.sisr_conv3x3_cin3(hip.ptr(dy), hip.ptr(w), 9, cin * 9, 1, None, hip.ptr(dx),
                                         hip.view_plain(H, W, cin), B, H, W, cin, hip.stream())
                hip.check(rc, "sisr_conv3x3_cin3(dgrad)")
            if need_w or need_b:
                dw = _grad_buf(w)
                db = _grad_buf(ctx.bias) if ctx.has_bias else None
                nbytes = L.sisr_corr3x3_c3_workspace_bytes(B, H, W, cin)
                ws = hip.workspace(dev, nbytes)
                rc = L.sisr_corr3x3_c3(hip.ptr(dy), hip.ptr(x), hip.view_plain(H, W, cin), 1.0, hip.ptr(dw), cin * 9, 9,
                                       1, 1, hip.ptr(db), hip.ptr(ws), nbytes, B, H, W, cin, hip.stream())
                hip.check(rc, "sisr_corr3x3_c3(tail)")
        return dx, dw, db, dres, None, None


def conv3x3(x, weight, bias=None, residual=None, alpha=1.0, shuffle=1):
    """y = conv3x3(x)*alpha + residual, optionally stored through PixelShuffle(shuffle)."""
    return _Conv3x3.apply(x, weight, bias, residual, float(alpha), int(shuffle))


# ----------------------------------------------------------------------------- meta gate (ParaCALayer FC stack)
class _MetaGate(Function):
    @staticmethod
    def forward(ctx, md, v1, c1, v2, c2, relu):
        B, M = md.shape[0], md.shape[1]
        md2 = md.reshape(B, M).contiguous()
        Hd, C = v1.shape[0], v2.shape[0]
        v1c, v2c = v1.reshape(Hd, M).contiguous(), v2.reshape(C, Hd).contiguous()
        hid, m = _vec(B, Hd, md.device), _vec(B, C, md.device)
        rc = hip.lib().sisr_meta_gate_fwd(hip.ptr(md2), B, M, Hd, C, hip.ptr(v1c), hip.ptr_c(c1),
                                          hip.ptr(v2c), hip.ptr_c(c2), int(relu), hip.ptr(hid), hip.ptr(m),
                                          hip.stream())
        hip.check(rc, "sisr_meta_gate_fwd")
        ctx.save_for_backward(md2, v1c, v2c, hid, m)
        ctx.relu, ctx.shapes = relu, (md.shape, v1.shape, v2.shape)
        return m

    @staticmethod
    def backward(ctx, dm):
        md2, v1c, v2c, hid, m = ctx.saved_tensors
        B, M = md2.shape
        Hd, C = v1c.shape[0], v2c.shape[0]
        dev = md2.device
        s_md, s_v1, s_v2 = ctx.shapes
        # allocated in the parameters' own shapes: a reshaped (view) gradient would be cloned by AccumulateGrad
        dv1, dc1 = torch.empty(s_v1, device=dev), torch.empty(Hd, device=dev)
        dv2, dc2 = torch.empty(s_v2, device=dev), torch.empty(C, device=dev)
        dmd = torch.empty_like(md2) if ctx.needs_input_grad[0] else None
        dmc, ws = dm.contiguous(), _vec(B, Hd + C, dev)  # named: temporaries of a call expression may share a block
        rc = hip.lib().sisr_meta_gate_bwd(hip.ptr(dmc), hip.ptr(m), hip.ptr(hid), hip.ptr(md2), B, M, Hd, C,
                                          hip.ptr(v1c), hip.ptr(v2c), int(ctx.relu), hip.ptr(dv1), hip.ptr(dc1),
                                          hip.ptr(dv2), hip.ptr(dc2), hip.ptr(dmd), hip.ptr(ws), hip.stream())
        hip.check(rc, "sisr_meta_gate_bwd")
        return (dmd.reshape(s_md) if dmd is not None else None, dv1, dc1, dv2, dc2, None)


def meta_gate(md, v1, c1, v2, c2, relu):
    """(B,M,1,1) metadata -> (B,C) sigmoid gate."""
    return _MetaGate.apply(md, v1, c1, v2, c2, bool(relu))


_meta_tables = {}


def _meta_table(params, device):
    """Device table [4][L] of the layers' (v1, c1, v2, c2) addresses, rebuilt when a parameter moved."""
    ptrs = tuple(t.data_ptr() for t in params)
    key = (device.index, len(ptrs))
    hit = _meta_tables.get(key)
    if hit is None or hit[0] != ptrs:
        L = len(ptrs) // 4
        tab = torch.tensor([[ptrs[4 * l + k] for l in range(L)] for k in range(4)], dtype=torch.int64).to(device)
        hit = (ptrs, tab)
        _meta_tables[key] = hit
    return hit[1]


class _MetaGateMany(Function):
    """The gates of L ParaCALayers (same M, hidden size, channel count, nonlinearity) in one launch each way:
    m[l] = sigmoid(V2_l act(V1_l md + c1_l) + c2_l)  ->  (L, B, C).  They depend on the metadata and the layers'
    own weights only, so a network computes all of them before its first block."""

    @staticmethod
    def forward(ctx, md, relu, *params):
        L = len(params) // 4
        B, M = md.shape[0], md.shape[1]
        if md.requires_grad:
            raise NotImplementedError("batched meta gates do not return a metadata gradient")
        for t in params:
            if not t.is_contiguous():
                raise NotImplementedError("batched meta gates need contiguous layer parameters")
        md2 = md.reshape(B, M).contiguous()
        Hd, C = params[0].shape[0], params[2].shape[0]
        dev = md.device
        tab = _meta_table(params, dev)
        hid = torch.empty((L, B, Hd), device=dev, dtype=torch.float32)
        m = torch.empty((L, B, C), device=dev, dtype=torch.float32)
        es = tab.element_size() * L
        base = tab.data_ptr()
        hip.check(hip.lib().sisr_meta_gate_many_fwd(hip.ptr(md2), B, M, Hd, C, L, base, base + es, base + 2 * es,
                                                    base + 3 * es, int(relu), hip.ptr(hid), hip.ptr(m), hip.stream()),
                  "sisr_meta_gate_many_fwd")
        ctx.save_for_backward(md2, hid, m, tab)
        ctx.cfg = (relu, L, B, M, Hd, C, [tuple(t.shape) for t in params[:4]])
        ctx.params = params  # the leaves themselves: their gradient sinks are looked up in backward
        return m

    @staticmethod
    def backward(ctx, dm):
        md2, hid, m, tab = ctx.saved_tensors
        relu, L, B, M, Hd, C, shapes = ctx.cfg
        dev = md2.device
        dmc = dm.contiguous()
        ws = torch.empty(L * B * (Hd + C), device=dev)
        es = tab.element_size() * L
        base = tab.data_ptr()
        keys = [t.data_ptr() for t in ctx.params]
        sinks = [GRAD_SINK.get(k) for k in keys]
        # the sinks take the FIRST gradient of a layer in a backward pass only (_grad_buf's contract): layers applied twice
        # (listed twice, or batched by two nodes of one pass) get private buffers, which autograd adds
        first = len(set(keys)) == len(keys)
        if _pass_id() >= 0:
            first = first and _PASS_BUFS.isdisjoint(keys)
            _PASS_BUFS.update(keys)
        if first and all(sk is not None and sk.shape == t.shape and t.grad is None for sk, t in zip(sinks, ctx.params)):
            # every gradient goes straight into the optimiser's arena (no gather before the update, no per-layer copy)
            gt = _meta_grad_table(sinks, dev)
            ges = gt.element_size() * L
            gb = gt.data_ptr()
            hip.check(hip.lib().sisr_meta_gate_many_bwd_scatter(hip.ptr(dmc), hip.ptr(m), hip.ptr(hid), hip.ptr(md2), B, M, Hd, C,
                                                                L, base, base + 2 * es, int(relu), gb, gb + ges, gb + 2 * ges,
                                                                gb + 3 * ges, hip.ptr(ws), hip.stream()),
                      "sisr_meta_gate_many_bwd_scatter")
            return (None, None, *[sk.detach() for sk in sinks])  # fresh aliases: autograd adopts what it alone holds
        dv1 = torch.empty((L,) + shapes[0], device=dev)
        dc1 = torch.empty((L,) + shapes[1], device=dev)
        dv2 = torch.empty((L,) + shapes[2], device=dev)
        dc2 = torch.empty((L,) + shapes[3], device=dev)
        hip.check(hip.lib().sisr_meta_gate_many_bwd(hip.ptr(dmc), hip.ptr(m), hip.ptr(hid), hip.ptr(md2), B, M, Hd, C, L,
                                                    base, base + 2 * es, int(relu), hip.ptr(dv1), hip.ptr(dc1),
                                                    hip.ptr(dv2), hip.ptr(dc2), hip.ptr(ws), hip.stream()),
                  "sisr_meta_gate_many_bwd")
        grads = []
        for l in range(L):  # row views: each is the only reference to its tensor object, so autograd adopts it
            grads += [dv1[l], dc1[l], dv2[l], dc2[l]]
        return (None, None, *grads)


_meta_grad_tables = {}


def _meta_grad_table(sinks, device):
    """Device table [4][L] of the layers' gradient-sink addresses (dv1, dc1, dv2, dc2), rebuilt when a sink moved."""
    ptrs = tuple(t.data_ptr() for t in sinks)
    key = (device.index, len(ptrs))
    hit = _meta_grad_tables.get(key)
    if hit is None or hit[0] != ptrs:
        L = len(ptrs) // 4
        tab = torch.tensor([[ptrs[4 * l + k] for l in range(L)] for k in range(4)], dtype=torch.int64).to(device)
        hit = (ptrs, tab)
        _meta_grad_tables[key] = hit
    return hit[1]


def meta_gate_many(md, layers, relu):
    """layers: [(v1, c1, v2, c2)] of L uniform ParaCALayers -> tuple of L (B, C) gates (views of one tensor)."""
    flat = [t for lay in layers for t in lay]
    return _MetaGateMany.apply(md, bool(relu), *flat).unbind(0)


class _GateMlp(Function):
    """The FC stack of a metadata-mixing QCALayer style on the pooled vector (csrc/attention.hip gate_mlp_*):
    (pool (B,C,1,1), metadata (B,M,1,1), optional meta gate (B,C)) -> gate (B,C,1,1)."""

    @staticmethod
    def forward(ctx, pool, md, mul, spec, *params):
        import ctypes
        layers, final_mode = spec  # layers: [(cat, relu_in, act)], params: w0, b0, w1, b1, ...
        B, C0 = pool.shape[0], pool.shape[1]
        M = md.shape[1]
        dev = pool.device
        L = len(layers)
        d = hip.GateMlpDesc()
        ws = [params[2 * k].reshape(params[2 * k].shape[0], -1).contiguous() for k in range(L)]
        bs = [params[2 * k + 1].contiguous() if params[2 * k + 1] is not None else None for k in range(L)]
        prev = C0
        for k, (cat, relu_in, act) in enumerate(layers):
            nout, inw = ws[k].shape
            if inw != prev + (M if cat else 0):
                raise RuntimeError(f"gate MLP layer {k}: weight expects {inw} inputs, got {prev + (M if cat else 0)}")
            d.w[k], d.b[k] = hip.ptr(ws[k]), hip.ptr(bs[k])
            d.nin[k], d.nout[k], d.cat[k], d.relu_in[k], d.act[k] = prev, nout, int(cat), int(relu_in), int(act)
            prev = nout
        d.L, d.M, d.C, d.final_mode = L, M, prev, final_mode
        p2, md2 = pool.reshape(B, C0).contiguous(), md.reshape(B, M).contiguous()
        mul2 = mul.reshape(B, prev).contiguous() if mul is not None else None
        aw = C0 + sum(w.shape[0] for w in ws)
        acts = torch.empty((B, aw), device=dev, dtype=torch.float32)
        yfin, y = _vec(B, prev, dev), _vec(B, prev, dev)
        hip.check(hip.lib().sisr_gate_mlp_fwd(hip.ptr(p2), hip.ptr(md2), hip.ptr(mul2), B, ctypes.addressof(d),
                                              hip.ptr(acts), hip.ptr(yfin), hip.ptr(y), hip.stream()), "sisr_gate_mlp_fwd")
        ctx.save_for_backward(md2, mul2, acts, yfin, *ws, *[b for b in bs if b is not None])
        ctx.cfg = (layers, final_mode, B, C0, M, prev, [tuple(params[2 * k].shape) for k in range(L)],
                   [b is not None for b in bs], tuple(pool.shape), tuple(md.shape),
                   tuple(mul.shape) if mul is not None else None)
        return y.reshape(B, prev, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        import ctypes
        layers, final_mode, B, C0, M, C, wshapes, has_b, s_pool, s_md, s_mul = ctx.cfg
        sv = list(ctx.saved_tensors)
        md2, mul2, acts, yfin = sv[:4]
        L = len(layers)
        ws = sv[4:4 + L]
        bs_present = sv[4 + L:]
        dev = acts.device
        d = hip.GateMlpDesc()
        prev, bi = C0, 0
        for k, (cat, relu_in, act) in enumerate(layers):
            d.w[k] = hip.ptr(ws[k])
            d.b[k] = hip.ptr(bs_present[bi]) if has_b[k] else None
            bi += int(has_b[k])
            d.nin[k], d.nout[k], d.cat[k], d.relu_in[k], d.act[k] = prev, ws[k].shape[0], int(cat), int(relu_in), int(act)
            prev = ws[k].shape[0]
        d.L, d.M, d.C, d.final_mode = L, M, C, final_mode
        dyc = dy.reshape(B, C).contiguous()
        zw = sum(w.shape[0] for w in ws)
        wsp = torch.empty((B, zw), device=dev, dtype=torch.float32)
        dpool = _vec(B, C0, dev)
        dmd = _vec(B, M, dev) if ctx.needs_input_grad[1] else None
        dmul = _vec(B, C, dev) if (mul2 is not None and ctx.needs_input_grad[2]) else None
        dws = [torch.empty(wshapes[k], device=dev, dtype=torch.float32) for k in range(L)]
        dbs = [torch.empty(ws[k].shape[0], device=dev, dtype=torch.float32) if has_b[k] else None for k in range(L)]
        PA = ctypes.c_void_p * hip.GM_MAXL
        dwa = PA(*[hip.ptr(t) for t in dws])
        dba = PA(*[hip.ptr(t) for t in dbs])
        hip.check(hip.lib().sisr_gate_mlp_bwd(hip.ptr(dyc), hip.ptr(md2), hip.ptr(mul2), B, ctypes.addressof(d),
                                              hip.ptr(acts), hip.ptr(yfin), hip.ptr(wsp), hip.ptr(dpool), hip.ptr(dmd),
                                              hip.ptr(dmul), dwa, dba, hip.stream()), "sisr_gate_mlp_bwd")
        grads = []
        for k in range(L):
            grads += [dws[k], dbs[k]]
        return (dpool.reshape(s_pool), dmd.reshape(s_md) if dmd is not None else None,
                dmul.reshape(s_mul) if dmul is not None else None, None, *grads)


# (cat metadata, ReLU on the concatenated input, activation 0 none / 1 relu / 2 sigmoid) per layer, final mode
QCA_STYLES = {
    "modulate": ([(0, 0, 1), (0, 0, 2)], 2),
    "max_concat": ([(1, 0, 1), (0, 0, 2)], 0),
    "softmax": ([(1, 0, 1), (0, 0, 2)], 1),
    "mini_concat": ([(0, 0, 0), (1, 1, 2)], 0),
    "extended_attention": ([(1, 0, 1), (1, 0, 1), (1, 0, 1), (0, 0, 2)], 0),
}


def qca_gate(pool, md, style, convs, mul=None):
    """convs: the style's nn.Conv2d 1x1 layers in order; mul: optional (B,C) meta-attention gate folded in."""
    params = []
    for c in convs:
        params += [c.weight, c.bias]
    return _GateMlp.apply(pool, md, mul, QCA_STYLES[style], *params)


# ----------------------------------------------------------------------------- fused residual block
class _ResBlock(Function):
    """y = x + gate * res_scale * conv2(relu(conv1(x)));  gate = CA(GAP(.)) [* m] | m | 1."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, caw1, cab1, caw2, cab2, m, res_scale):
        B, C, H, W = x.shape
        has_ca, has_m = caw1 is not None, m is not None
        if C % 64 or tuple(w1.shape) != (C, C, 3, 3) or tuple(w2.shape) != (C, C, 3, 3):
            raise NotImplementedError("fused residual block needs n_feats to be a multiple of 64")
        if C != 64 and (has_ca or has_m):
            raise NotImplementedError("the gated residual blocks (RCAB / QRCAB / ParamResBlock) are specialised for "
                                      "n_feats = 64; the plain ResBlock runs at any multiple of 64 (EDSR 256)")
        _join_pending.clear()  # a backward pass that died mid-way must not leave the join flag set
        dev = x.device
        x = _cl(x)
        w1, w2 = w1.contiguous(), w2.contiguous()
        v = hip.view_plain(H, W, C)
        t1 = _empty_cl(B, C, H, W, dev)
        if any(ctx.needs_input_grad):
            p1, ctx.pd1 = pack_pair(w1)
            p2, ctx.pd2 = pack_pair(w2)
        else:
            p1, p2 = pack_weight(w1, "fwd"), pack_weight(w2, "fwd")
        conv_c64(x, v, p1, b1, (1, 64), t1, v, B, H, W, C, C, relu=True)
        y = _empty_cl(B, C, H, W, dev)
        saved_vecs = []
        if not has_ca and not has_m:  # ResBlock: everything fuses into conv2's epilogue
            conv_c64(t1, v, p2, b2, (1, 64), y, v, B, H, W, C, C, res=x, alpha=res_scale)
            t2 = None
        else:
            t2 = _empty_cl(B, 64, H, W, dev)
            if has_ca:
                parts = gap_parts(H, W)
                gap = torch.empty((B, parts, 64), device=dev, dtype=torch.float32)
                conv_c64(t1, v, p2, b2, (1, 64), t2, v, B, H, W, 64, 64, alpha=res_scale, gap=gap)
                R = caw1.shape[0]
                caw1c, caw2c = caw1.reshape(R, 64).contiguous(), caw2.reshape(64, R).contiguous()
                s, hid, ca, g = _vec(B, 64, dev), _vec(B, R, dev), _vec(B, 64, dev), _vec(B, 64, dev)
                mm = m.contiguous() if has_m else None
                rc = hip.lib().sisr_ca_gate_fwd(hip.ptr(gap), parts, B, 1.0 / (H * W), hip.ptr(caw1c),
                                                hip.ptr_c(cab1), hip.ptr(caw2c), hip.ptr_c(cab2),
                                                64, R, hip.ptr(mm), hip.ptr(s), hip.ptr(hid), hip.ptr(ca), hip.ptr(g),
                                                hip.stream())
                hip.check(rc, "sisr_ca_gate_fwd")
                saved_vecs = [caw1c, caw2c, s, hid, ca, g] + ([mm] if has_m else [])
            else:
                conv_c64(t1, v, p2, b2, (1, 64), t2, v, B, H, W, 64, 64, alpha=res_scale)
                g = m.contiguous()
                saved_vecs = [g]
            rc = hip.lib().sisr_gate_residual_fwd(hip.ptr(t2), hip.ptr(g), None, hip.ptr(x), hip.ptr(y), B, H * W, 64,
                                                  hip.stream())
            hip.check(rc, "sisr_gate_residual_fwd")
        ctx.save_for_backward(x, w1, w2, t1, *([t2] if t2 is not None else []), *saved_vecs)
        ctx.cfg = (has_ca, has_m, float(res_scale), (B, H, W), tuple(caw1.shape) if has_ca else None,
                   tuple(caw2.shape) if has_ca else None)
        return y

    @staticmethod
    @_in_backward
    def backward(ctx, dy):
        has_ca, has_m, rs, (B, H, W), s_caw1, s_caw2 = ctx.cfg
        sv = list(ctx.saved_tensors)
        x, w1, w2, t1 = sv[:4]
        C = x.shape[1]  # 64 for the gated modes; any multiple of 64 for the plain ResBlock
        dev = x.device
        L = hip.lib()
        dy = _cl(dy)
        v = hip.view_plain(H, W, C)
        hw = H * W
        dcaw1 = dcab1 = dcaw2 = dcab2 = dm = None
        scale = shift = None
        if has_ca or has_m:
            t2 = sv[4]
            parts = L.sisr_gate_dg_parts(hw)
            dgp = torch.empty((B, parts, 64), device=dev, dtype=torch.float32)
            hip.check(L.sisr_gate_dg_partial(hip.ptr(dy), hip.ptr(t2), hip.ptr(dgp), B, hw, 64, hip.stream()),
                      "sisr_gate_dg_partial")
            if has_ca:
                caw1c, caw2c, s, hid, ca, g = sv[5:11]
                mm = sv[11] if has_m else None
                R = caw1c.shape[0]
                shift = _vec(B, 64, dev)
                dmv = _vec(B, 64, dev) if has_m else None
                dcaw1, dcab1 = torch.empty(s_caw1, device=dev), torch.empty(R, device=dev)
                dcaw2, dcab2 = torch.empty(s_caw2, device=dev), torch.empty(64, device=dev)
                rc = L.sisr_ca_gate_bwd(hip.ptr(dgp), parts, B, 1.0 / hw, hip.ptr(caw1c), hip.ptr(caw2c), 64, R,
                                        hip.ptr(s), hip.ptr(hid), hip.ptr(ca), hip.ptr(mm), hip.ptr(shift),
                                        hip.ptr(dmv), hip.ptr(dcaw1), hip.ptr(dcab1), hip.ptr(dcaw2), hip.ptr(dcab2),
                                        hip.ptr(_gate_ws(B, dev)), hip.gate_counter(dev), hip.stream())
                hip.check(rc, "sisr_ca_gate_bwd")
                dm, scale = dmv, g
            else:
                g = sv[5]
                dm = _vec(B, 64, dev)
                hip.check(L.sisr_sum_partials(hip.ptr(dgp), parts, B, 64, 1.0, hip.ptr(dm), hip.stream()),
                          "sisr_sum_partials")
                scale = g
        # conv2 backward: dt2 = dy*scale + shift is rebuilt on load, never stored
        # plain first-order backward only; not under hipGraph capture (record_stream + private pools)
        side = _side_ok(w1, w2, pixels=B * H * W)
        dw2, db2 = _grad_buf(w2, _PASS_ID), torch.empty(C, device=dev)
        dw1, db1 = _grad_buf(w1, _PASS_ID), torch.empty(C, device=dev)

        def wgrad2():
            wgrad_c64(t1, v, dy, v, dw2, db2, B, H, W, C, C, alpha=rs, dy_scale=scale, dy_shift=shift, owner=w2)

        if side:
            _side_launch(dev, wgrad2, (t1, dy, scale, shift, dw2, db2))
        dt1 = _empty_cl(B, C, H, W, dev)
        conv_c64(dy, v, ctx.pd2, None, (1, 64), dt1, v, B, H, W, C, C, mask=t1, in_scale=scale, in_shift=shift,
                 alpha=rs)
        if not side:
            wgrad2()

        def wgrad1():
            wgrad_c64(x, v, dt1, v, dw1, db1, B, H, W, C, C, owner=w1)

        # conv1 backward (+ skip connection gradient)
        if side:
            _side_launch(dev, wgrad1, (x, dt1, dw1, db1))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty_cl(B, C, H, W, dev)
            conv_c64(dt1, v, ctx.pd1, None, (1, 64), dx, v, B, H, W, C, C, res=dy)
        if not side:
            wgrad1()
        return dx, dw1, db1, dw2, db2, dcaw1, dcab1, dcaw2, dcab2, (dm if has_m else None), None


LANES = 1  # bench.py reports this as `sample_lanes`: one launch chain per residual group (sample lanes tied and were removed)


class _GatedGroup(Function):
    """A whole residual group of channel-attention blocks as ONE autograd node:

        out = x + conv_t(u_n),   u_k = u_{k-1} + g_k * conv2_k(relu(conv1_k(u_{k-1}))),   u_0 = x,
        g_k = sigmoid(CA_k(mean_hw(conv2_k(..)))) [* m_k]          (ref: advanced/architectures.py:68-71, :107-110;
                                                                    attention_manipulators/architectures.py:172-180, :229-233)

    Same kernels and arithmetic as the per-block node, but the two passes a block cannot fuse on its own move into
    its neighbours: the gated skip  u_k = t2_k * g_k + u_{k-1}  is built (and written once) by the NEXT conv's
    halo staging, and the gate gradient  sum(dU_k * t2_k)  is taken by the PREVIOUS backward conv's epilogue while
    it produces dU_k.  Per block that removes two HBM-bound launches (3 + 2 map passes with the MFMA units idle).

    Both passes are one chain of launches over the whole batch on the calling stream.  The channel-attention gate (and its
    backward) is a launch of its own between two convs, or, while launches are small (GATE_HEADS), a head of the conv that
    consumes it."""

    PER = 9  # w1, b1, w2, b2, caw1, cab1, caw2, cab2, m

    @staticmethod
    def forward(ctx, x, n, alpha, *args):
        B, C, H, W = x.shape
        if C != 64:
            raise NotImplementedError("fused residual group is specialised for n_feats = 64")
        # Blocks WITHOUT channel attention (QEDSR's ParamResBlock, ref attention_manipulators/architectures.py:348-356:
        # x + m * (res_scale * conv2(relu(conv1 x)))): the gate is the meta-attention vector alone, known before the first
        # launch -- no pooling, no gate launch; `alpha` = res_scale rides in conv2's epilogue.  All blocks of a group alike.
        has_ca = args[4] is not None
        if not has_ca and args[8] is None:
            raise NotImplementedError("fused residual group: a block needs a channel-attention gate or a meta gate")
        alpha = float(alpha)
        _join_pending.clear()
        dev, L = x.device, hip.lib()
        x = _cl(x)
        v = hip.view_plain(H, W, 64)
        need = any(ctx.needs_input_grad)
        parts = gap_parts(H, W)
        heads = has_ca and GATE_HEADS and WgradQueue.wanted(B, H, W) and B * H * W <= GATE_HEADS_MAX_PIXELS
        PER = _GatedGroup.PER
        # bf16 operand mode with bf16 storage: the maps this group keeps (t1, t2, the gated skips) are bf16 in HBM
        st16 = PRECISION == "bf16" and BF16_STORAGE in ("act", "all") and not heads
        new_map = _empty_cl16 if st16 else _empty_cl
        x_in = to_bf16_map(x) if st16 else x  # block 0's input and first skip, in the group's storage format

        def conv(xx, pk, bias, yy, storage, head=None, **kw):
            if st16:  # (no gate heads there)
                conv_c64s(xx, pk, bias, yy, B, H, W, storage, **kw)
            else:
                conv_c64(xx, v, pk, bias, (1, 64), yy, v, B, H, W, 64, 64, ca_head=head, **kw)

        def pack(w):
            return pack_pair(w) if need else (pack_weight(w, "fwd"), None)

        # every buffer of the group, on the calling stream
        blks, tensors, packs, meta, small = [], [], [], [], []
        if not has_ca and alpha != 1.0:  # alpha * m of every block in two launches
            gs_all = torch.stack([args[k * PER + 8] for k in range(n)]).mul_(alpha)
        for k in range(n):
            w1, b1, w2, b2, caw1, cab1, caw2, cab2, m = args[k * PER:(k + 1) * PER]
            w1, w2 = w1.contiguous(), w2.contiguous()
            p1, pd1 = pack(w1)
            p2, pd2 = pack(w2)
            if has_ca:
                R = caw1.shape[0]
                d = dict(p1=p1, p2=p2, b1=b1, b2=b2, R=R, t1=new_map(B, 64, H, W, dev), t2=new_map(B, 64, H, W, dev),
                         u=new_map(B, 64, H, W, dev) if k > 0 else x_in,
                         gap=torch.empty((B, parts, 64), device=dev, dtype=torch.float32),
                         caw1c=caw1.reshape(R, 64).contiguous(), caw2c=caw2.reshape(64, R).contiguous(),
                         cb1=cab1.contiguous(), cb2=cab2.contiguous(), mm=m.contiguous() if m is not None else None,
                         sv=_vec(B, 64, dev), hid=_vec(B, R, dev), ca=_vec(B, 64, dev), g=_vec(B, 64, dev))
                blk = [d["u"], w1, w2, d["t1"], d["t2"], d["caw1c"], d["caw2c"], d["sv"], d["hid"], d["ca"], d["g"]]
                if d["mm"] is not None:
                    blk.append(d["mm"])
                meta.append((len(blk), d["mm"] is not None))
            else:
                mm = m.contiguous()
                # gs = alpha * m: the scale of the gradient entering conv2 (its input gradient and its weight gradient both
                # rebuild dt2 = dU * gs while staging, so both run with alpha = 1 and the weight gradient stays batchable)
                d = dict(p1=p1, p2=p2, b1=b1, b2=b2, R=0, t1=new_map(B, 64, H, W, dev), t2=new_map(B, 64, H, W, dev),
                         u=new_map(B, 64, H, W, dev) if k > 0 else x_in, gap=None, mm=mm, g=mm,
                         gs=mm if alpha == 1.0 else gs_all[k], sv=None, hid=None, ca=None)
                blk = [d["u"], w1, w2, d["t1"], d["t2"], d["g"], d["gs"]]
                meta.append((len(blk), True))
            blks.append(d)
            small.append((b1, b2, caw1, cab1, caw2, cab2))
            tensors += blk
            packs.append((pd1, pd2))
        wt, bt = args[n * PER:n * PER + 2]
        wt = wt.contiguous()
        pt, pdt = pack(wt)
        un, out = new_map(B, 64, H, W, dev), _empty_cl(B, 64, H, W, dev)

        pend = None  # (t2, g, gate head) of the block whose gated skip the next conv builds
        for k in range(n):
            d = blks[k]
            if pend is None:
                conv(x_in, d["p1"], d["b1"], d["t1"], 3, relu=True)
            else:
                conv(pend[0], d["p1"], d["b1"], d["t1"], 3, head=pend[2], relu=True, in_scale=pend[1],
                     gate_add=blks[k - 1]["u"], gate_out=d["u"])
            hd = None
            if not has_ca:  # the gate is the meta-attention vector: nothing to pool, nothing to launch
                conv(d["t1"], d["p2"], d["b2"], d["t2"], 3, alpha=alpha)
            else:
                conv(d["t1"], d["p2"], d["b2"], d["t2"], 3, gap=d["gap"])
                if heads:  # the gate is computed by the conv that consumes it (the next block's conv1, or the group's tail conv)
                    hd = hip.CaTail()  # copied into the launch's arguments: it need not outlive the call
                    hd.backward, hd.hidden, hd.inv_hw, hd.head, hd.head_parts = 0, d["R"], 1.0 / (H * W), 1, parts
                    hd.w1, hd.b1, hd.w2, hd.b2, hd.mul = (hip.ptr(d["caw1c"]), hip.ptr(d["cb1"]), hip.ptr(d["caw2c"]),
                                                          hip.ptr(d["cb2"]), hip.ptr(d["mm"]))
                    hd.s_out, hd.hid_out, hd.ca_out, hd.g_out = hip.ptr(d["sv"]), hip.ptr(d["hid"]), hip.ptr(d["ca"]), hip.ptr(d["g"])
                    hd.head_part = hip.ptr(d["gap"])
                else:
                    hip.check(L.sisr_ca_gate_fwd(hip.ptr(d["gap"]), parts, B, 1.0 / (H * W), hip.ptr(d["caw1c"]), hip.ptr(d["cb1"]),
                                                 hip.ptr(d["caw2c"]), hip.ptr(d["cb2"]), 64, d["R"], hip.ptr(d["mm"]),
                                                 hip.ptr(d["sv"]), hip.ptr(d["hid"]), hip.ptr(d["ca"]), hip.ptr(d["g"]),
                                                 hip.stream()), "sisr_ca_gate_fwd")
            pend = (d["t2"], d["g"], hd)
        # (st16: bf16 t2 and skips in, the group's output, with its fp32 input as the residual, in fp32)
        conv(pend[0], pt, bt, out, 1, head=pend[2], in_scale=pend[1], gate_add=blks[n - 1]["u"], gate_out=un, res=x)
        ctx.save_for_backward(*tensors, un, wt)
        ctx.cfg = (n, (B, H, W), meta, parts)
        ctx.packs, ctx.pdt = packs, pdt
        ctx.small, ctx.bt = small, bt  # the small parameters: their gradients go straight into the optimiser's arena too
        ctx.st16, ctx.grad16 = st16, st16 and BF16_STORAGE == "all"
        ctx.has_ca = has_ca
        return out

    @staticmethod
    @_in_backward
    def backward(ctx, dout):
        n, (B, H, W), meta, parts = ctx.cfg
        sv_all = list(ctx.saved_tensors)
        un, wt = sv_all[-2], sv_all[-1]
        dev, L = un.device, hip.lib()
        v = hip.view_plain(H, W, 64)
        hw = H * W
        dout = _cl(dout)

        def run(fn, keep):
            _side_launch(dev, fn, keep, side)

        blocks, pos = [], 0
        for cnt, has_m in meta:
            blocks.append((sv_all[pos:pos + cnt], has_m))
            pos += cnt
        # st16: the saved activations (un, every block's input, t1, t2) are bf16 maps; g16: so are the gradient maps the
        # launches of this pass hand to each other (the group's own input / output gradients stay fp32)
        st16, g16 = ctx.st16, ctx.grad16
        has_ca = ctx.has_ca
        wst = 1 if st16 else 0
        grad_map = _empty_cl16 if g16 else _empty_cl

        def conv(xx, pk, yy, head=None, **kw):
            """a backward conv of the group; under st16 bf16 mask / dot operands and storage bits from the maps' own dtypes"""
            st = ((1 if xx.dtype == torch.bfloat16 else 0) | (2 if yy.dtype == torch.bfloat16 else 0) |
                  (4 if (kw.get("mask") is not None or kw.get("dot") is not None) else 0) |
                  (8 if (kw.get("res") is not None and kw["res"].dtype == torch.bfloat16) else 0)) if st16 else 0
            if st:  # (no gate heads there)
                conv_c64s(xx, pk, None, yy, B, H, W, st, **kw)
            else:
                conv_c64(xx, v, pk, None, (1, 64), yy, v, B, H, W, 64, 64, ca_head=head, **kw)

        side = _side_ok(wt, *(t for blk in blocks for t in blk[0][1:3]))
        # small launches: the group's 2n + 1 weight gradients go out eight to a launch (WgradQueue) instead of one by one
        queue = WgradQueue(B, H, W, dev) if WgradQueue.wanted(B, H, W) else None
        bheads = has_ca and queue is not None and GATE_HEADS and B * H * W <= GATE_HEADS_MAX_PIXELS
        gate_jobs = []
        # tail conv: weight gradient from (u_n, dout); dU_n = convT(dout), with sum(dU_n * t2_n) on the side
        gid = _PASS_ID  # _side_ok has just asked: one look at the graph task for the group's ~8n gradient buffers
        dwt, dbt = _grad_buf(wt, gid), _grad_buf_or(ctx.bt, 64, dev, gid)
        if queue is not None:
            queue.add(un, dout, dwt, dbt)
        else:
            run(lambda: wgrad_c64(un, v, dout, v, dwt, dbt, B, H, W, 64, 64, storage=wst), (un, dout, dwt, dbt))

        def gate_bwd_out(k):
            """Outputs of block k's gate backward (allocated before the conv launch whose head fills them)."""
            has_m = blocks[k][1]
            _, _, caw1, cab1, caw2, cab2 = ctx.small[k]
            if not has_ca:  # the meta gate's gradient is the sum of the DOT partials; no pooling gradient, no CA parameters
                return dict(shift=None, dmv=_vec(B, 64, dev), dcaw1=None, dcab1=None, dcaw2=None, dcab2=None, dzw=None,
                            dgp=torch.empty((B, parts, 64), device=dev, dtype=torch.float32))
            return dict(shift=_vec(B, 64, dev), dmv=_vec(B, 64, dev) if has_m else None,
                        dcaw1=_grad_buf(caw1, gid), dcab1=_grad_buf(cab1, gid), dcaw2=_grad_buf(caw2, gid),
                        dcab2=_grad_buf(cab2, gid),
                        dgp=torch.empty((B, parts, 64), device=dev, dtype=torch.float32),
                        dzw=torch.empty((B, 80), device=dev) if queue is not None else None)

        grads = [None] * (n * _GatedGroup.PER)

        def wgrad2(k, dy, go):
            """Weight gradient of block k's second conv, from (t1, the gated gradient dy * g + shift rebuilt while staging)."""
            tens = blocks[k][0]
            w2, t1, g = tens[2], tens[3], tens[10] if has_ca else tens[6]
            dw2, db2 = _grad_buf(w2, gid), _grad_buf_or(ctx.small[k][1], 64, dev, gid)
            shift = go["shift"]
            if queue is not None:
                queue.add(t1, dy, dw2, db2, dy_scale=g, dy_shift=shift)
            else:
                run(lambda: wgrad_c64(t1, v, dy, v, dw2, db2, B, H, W, 64, 64, dy_scale=g, dy_shift=shift,
                                      storage=3 if g16 else wst), (t1, dy, g, shift, dw2, db2))
            grads[k * _GatedGroup.PER + 2:k * _GatedGroup.PER + 4] = [dw2, db2]

        def wgrad1(k, go, dt1):
            """Weight gradient of block k's first conv, from (the block's input, dt1); the block's small gradients."""
            tens, has_m = blocks[k]
            xk, w1 = tens[0], tens[1]
            caw1c, s, hid = (tens[5], tens[7], tens[8]) if has_ca else (None, None, None)
            dw1, db1 = _grad_buf(w1, gid), _grad_buf_or(ctx.small[k][0], 64, dev, gid)
            if queue is not None:
                if has_ca:
                    gate_jobs.append((go["dzw"], hid, s, go["dcaw1"], go["dcab1"], go["dcaw2"], go["dcab2"], caw1c.shape[0]))
                queue.add(xk, dt1, dw1, db1)
            else:
                run(lambda: wgrad_c64(xk, v, dt1, v, dw1, db1, B, H, W, 64, 64, storage=3 if g16 else wst),
                    (xk, dt1, dw1, db1))
            P = _GatedGroup.PER
            grads[k * P:k * P + 2] = [dw1, db1]
            grads[k * P + 4:k * P + 9] = [go["dcaw1"], go["dcab1"], go["dcaw2"], go["dcab2"], go["dmv"] if has_m else None]

        # dU_n = convT_tail(dout), with the partial sums of sum(dU_n * t2_n) for block n - 1's gate backward
        dy = grad_map(B, 64, H, W, dev)
        go = gate_bwd_out(n - 1)
        conv(dout, ctx.pdt, dy, gap=go["dgp"], dot=blocks[-1][0][4])
        for k in range(n - 1, -1, -1):
            # block k: gate backward (a launch, or a head of the next conv), dgrad through conv2 (ReLU mask, gated gradient
            # rebuilt while staging), dgrad through conv1 (+ the skip's gradient; partial sums for block k - 1's gate
            # backward).  Its maps come and go block by block; its weight gradients follow their operands
            tens, has_m = blocks[k]
            pd1, pd2 = ctx.packs[k]
            dt1 = grad_map(B, 64, H, W, dev)  # gradient at ReLU(conv1)
            dprev = (grad_map if k > 0 else _empty_cl)(B, 64, H, W, dev)  # gradient at the block's input
            gn = gate_bwd_out(k - 1) if k > 0 else None  # block k - 1's gate backward, which block k's last conv feeds
            t1 = tens[3]
            bhead = None
            if not has_ca:
                hip.check(L.sisr_sum_partials(hip.ptr(go["dgp"]), parts, B, 64, 1.0, hip.ptr(go["dmv"]), hip.stream()),
                          "sisr_sum_partials")
                g, shift = tens[6], None  # dt2 = dU * (alpha * m)
            else:
                caw1c, caw2c, s, hid, ca, g = tens[5:11]
                mm = tens[11] if has_m else None
                R = caw1c.shape[0]
                shift, dmv = go["shift"], go["dmv"]
                if bheads:  # the per-sample part of the gate backward is computed by the conv that consumes `shift`
                    bhead = hip.CaTail()
                    bhead.backward, bhead.hidden, bhead.inv_hw, bhead.head, bhead.head_parts = 1, R, 1.0 / hw, 1, parts
                    bhead.w1, bhead.w2, bhead.hid, bhead.ca, bhead.mul = (hip.ptr(caw1c), hip.ptr(caw2c), hip.ptr(hid),
                                                                          hip.ptr(ca), hip.ptr(mm))
                    bhead.shift, bhead.dmul, bhead.workspace, bhead.head_part = (hip.ptr(shift), hip.ptr(dmv),
                                                                                  hip.ptr(go["dzw"]), hip.ptr(go["dgp"]))
                elif queue is not None:
                    # small launches: the chain kernel only produces what the next conv waits for; the gates' parameter
                    # gradients of the whole group are one launch at the end (their dz2 / dz1 wait in per-gate workspaces)
                    hip.check(L.sisr_ca_gate_bwd(hip.ptr(go["dgp"]), parts, B, 1.0 / hw, hip.ptr(caw1c), hip.ptr(caw2c), 64,
                                                 R, hip.ptr(s), hip.ptr(hid), hip.ptr(ca), hip.ptr(mm), hip.ptr(shift),
                                                 hip.ptr(dmv), None, None, None, None, hip.ptr(go["dzw"]), None,
                                                 hip.stream()), "sisr_ca_gate_bwd")
                else:
                    hip.check(L.sisr_ca_gate_bwd(hip.ptr(go["dgp"]), parts, B, 1.0 / hw, hip.ptr(caw1c), hip.ptr(caw2c), 64,
                                                 R, hip.ptr(s), hip.ptr(hid), hip.ptr(ca), hip.ptr(mm), hip.ptr(shift),
                                                 hip.ptr(dmv), hip.ptr(go["dcaw1"]), hip.ptr(go["dcab1"]),
                                                 hip.ptr(go["dcaw2"]), hip.ptr(go["dcab2"]), hip.ptr(_gate_ws(B, dev)),
                                                 hip.gate_counter(dev), hip.stream()), "sisr_ca_gate_bwd")
            if queue is None:  # side stream: wgrad2 beside conv2's input gradient, wgrad1 beside conv1's
                wgrad2(k, dy, go)
            conv(dy, pd2, dt1, head=bhead, mask=t1, in_scale=g, in_shift=shift)
            if queue is not None:  # queued: after the block's first conv (with a gate head it is that launch which fills `shift`)
                wgrad2(k, dy, go)
            wgrad1(k, go, dt1)
            if k > 0:
                conv(dt1, pd1, dprev, res=dy, gap=gn["dgp"], dot=blocks[k - 1][0][4])
            else:  # (g16: bf16 in, bf16 residual, the group's fp32 dX out)
                conv(dt1, pd1, dprev, res=dy)
            dy, go = dprev, gn
        dx = _affine(dy, None, None, dout, B, H, W, 64) if ctx.needs_input_grad[0] else None
        if queue is not None:
            queue.flush()  # before the gradients leave the node (reducer hooks may read them right after)
            import ctypes
            cap = L.sisr_ca_gate_bwd_params_batch_max()
            for i0 in range(0, len(gate_jobs), cap):
                chunk = gate_jobs[i0:i0 + cap]
                arr = (hip.CaParamJob * len(chunk))()
                for k, (dzw, hid, s, a1, c1, a2, c2, _) in enumerate(chunk):
                    arr[k].dz, arr[k].hid, arr[k].s = hip.ptr(dzw), hip.ptr(hid), hip.ptr(s)
                    arr[k].dw1, arr[k].db1, arr[k].dw2, arr[k].db2 = hip.ptr(a1), hip.ptr(c1), hip.ptr(a2), hip.ptr(c2)
                hip.check(L.sisr_ca_gate_bwd_params_batch(ctypes.addressof(arr), len(chunk), B, chunk[0][7], hip.stream()),
                          "sisr_ca_gate_bwd_params_batch")
        return (dx, None, None, *grads, dwt, dbt)


def gated_group(x, blocks, tail_w, tail_b, alpha=1.0):
    """blocks: list of (w1, b1, w2, b2, (caw1, cab1, caw2, cab2) or None, m or None); alpha: scale of every block's second conv
    (res_scale); see _GatedGroup."""
    flat = []
    for w1, b1, w2, b2, ca, m in blocks:
        flat += [w1, b1, w2, b2, *(ca if ca is not None else (None,) * 4), m]
    return _GatedGroup.apply(x, len(blocks), float(alpha), *flat, tail_w, tail_b)


def fused_groups_enabled():
    """Group-level node (GATE / DOT conv variants) on or off; SISR_FUSED_GROUPS=0 keeps the per-block nodes."""
    return FUSED_GROUPS


def res_block(x, w1, b1, w2, b2, ca=None, m=None, res_scale=1.0):
    """ca = (w1,b1,w2,b2) of the CA squeeze/excite 1x1 convs or None; m = (B,64) meta gate or None."""
    if x.shape[1] != 64 and (ca is not None or m is not None):
        return _wide_gated_block(x, w1, b1, w2, b2, ca, m, float(res_scale))
    caw1, cab1, caw2, cab2 = ca if ca is not None else (None, None, None, None)
    return _ResBlock.apply(x, w1, b1, w2, b2, caw1, cab1, caw2, cab2, m, float(res_scale))


class _ConvReluConv(Function):
    """t2 = alpha * conv2(relu(conv1(x))) without gate/skip (the metadata-mixing QCALayer styles; gated blocks wider than 64
    channels); any multiple of 64 channels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, alpha):
        B, C, H, W = x.shape
        if C % 64 or tuple(w1.shape) != (C, C, 3, 3) or tuple(w2.shape) != (C, C, 3, 3):
            raise NotImplementedError("fused conv pair needs n_feats to be a multiple of 64")
        x = _cl(x)
        w1, w2 = w1.contiguous(), w2.contiguous()
        v = hip.view_plain(H, W, C)
        t1, t2 = _empty_cl(B, C, H, W, x.device), _empty_cl(B, C, H, W, x.device)
        conv_c64(x, v, pack_weight(w1, "fwd"), b1, (1, 64), t1, v, B, H, W, C, C, relu=True)
        conv_c64(t1, v, pack_weight(w2, "fwd"), b2, (1, 64), t2, v, B, H, W, C, C, alpha=alpha)
        ctx.save_for_backward(x, w1, w2, t1)
        ctx.alpha, ctx.b1, ctx.b2 = alpha, b1, b2
        return t2

    @staticmethod
    @_in_backward
    def backward(ctx, dt2):
        x, w1, w2, t1 = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        dt2 = _cl(dt2)
        v = hip.view_plain(H, W, C)
        dt1 = _empty_cl(B, C, H, W, dev)
        conv_c64(dt2, v, pack_weight(w2, "dgrad"), None, (1, 64), dt1, v, B, H, W, C, C, mask=t1, alpha=ctx.alpha)
        dw2, db2 = _grad_buf(w2), _grad_buf_or(ctx.b2, C, dev)
        wgrad_c64(t1, v, dt2, v, dw2, db2, B, H, W, C, C, alpha=ctx.alpha, owner=w2)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty_cl(B, C, H, W, dev)
            conv_c64(dt1, v, pack_weight(w1, "dgrad"), None, (1, 64), dx, v, B, H, W, C, C)
        dw1, db1 = _grad_buf(w1), _grad_buf_or(ctx.b1, C, dev)
        wgrad_c64(x, v, dt1, v, dw1, db1, B, H, W, C, C, owner=w1)
        return dx, dw1, db1, dw2, db2, None


def res_block_convs(x, w1, b1, w2, b2, alpha=1.0):
    return _ConvReluConv.apply(x, w1, b1, w2, b2, float(alpha))


def _wide_gated_block(x, w1, b1, w2, b2, ca, m, res_scale):
    """RCAB / QRCAB('standard') / ParamResBlock at n_feats = 128, 192, 256, ... (ref: attention_manipulators/handlers.py:24-29
    forwards n_feats to QRCAN): the same arithmetic from the modular operators -- conv pair on the multi-chunk MFMA kernels,
    ordered pixel sums, the squeeze / excite MLP on the generic gate kernel (one workgroup per sample), gate * t2 + x --
    instead of the 64-channel fused node."""
    B, C = x.shape[0], x.shape[1]
    t2 = res_block_convs(x, w1, b1, w2, b2, alpha=res_scale)
    if ca is not None:
        caw1, cab1, caw2, cab2 = ca
        pool = global_avg_pool(t2)
        md0 = x.new_zeros((B, 1, 1, 1))  # the plain squeeze / excite stack concatenates no metadata
        g = _GateMlp.apply(pool, md0, m, ([(0, 0, 1), (0, 0, 2)], 0), caw1, cab1, caw2, cab2)
    else:
        g = m
    return gate_mul(t2, g.reshape(B, C, 1, 1), x)


# ----------------------------------------------------------------------------- helpers and codes more than one family uses
def _pad64(n):
    return (n + 63) // 64 * 64


def _pad_oihw(w, cop, cip):
    """(co, ci, kh, kw) -> zero-padded (cop, cip, kh, kw) copy (the weight itself when nothing is to pad)."""
    co, ci = w.shape[0], w.shape[1]
    if co == cop and ci == cip:
        return w.contiguous()
    taps = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
    out = torch.empty((cop, cip) + tuple(w.shape[2:]), device=w.device, dtype=torch.float32)
    hip.check(hip.lib().sisr_pad_oihw(hip.ptr(w.contiguous()), hip.ptr(out), co, ci, cop, cip, taps, 0, hip.stream()),
              "sisr_pad_oihw")
    return out


def _crop_oihw(wp, shape):
    """Inverse of _pad_oihw for gradients."""
    if tuple(wp.shape) == tuple(shape):
        return wp
    co, ci = shape[0], shape[1] if len(shape) > 1 else 1
    taps = shape[2] * shape[3] if len(shape) == 4 else 1
    out = torch.empty(shape, device=wp.device, dtype=torch.float32)
    hip.check(hip.lib().sisr_pad_oihw(hip.ptr(wp), hip.ptr(out), co, ci, wp.shape[0], wp.shape[1] if wp.dim() > 1 else 1,
                                      taps, 1, hip.stream()), "sisr_pad_oihw(crop)")
    return out


# SPARNet's stride-1 ConvLayer convs with reflection / nearest upsampling inside the MFMA kernels' staging (0: the gather ->
# conv -> gather composition of round 3, kept for the stride-2 convs and as the A/B reference; results are bit-identical)
REFL_GEO = os.environ.get("SISR_REFL_GEO", "1") != "0"
REFL_BATCH = os.environ.get("SISR_REFL_BATCH", "1") != "0"  # their small weight gradients eight per launch (WgradGeoQueue)

LEAKY, LEAKY_MASK = 2, 4  # `relu` codes of sisr_conv3x3_c64: LeakyReLU(0.2) epilogue / the mask is its derivative
SPARSE_BLOCK_DIAGONAL, SPARSE_SECOND_CHUNK, SPARSE_HALVES = 8, 9, 10  # `select` codes: structural zeros of the merged SFT weights are skipped


def _fp32_only(what):
    if PRECISION != "fp32":
        raise NotImplementedError(f"{what} runs on the fp32 kernels only (SISR_PRECISION={PRECISION})")


def _map64(a, a_stride, b, b_stride, out, out_stride, npix, op, a_off=0, out_off=0):
    """op 0 copy / 1 a + b / 2 LeakyReLU(a) / 3 b * LeakyReLU'(a) on 64-channel maps with pixel strides (floats)."""
    hip.check(hip.lib().sisr_map64(hip.ptr(a) + 4 * a_off, a_stride, hip.ptr(b), b_stride, hip.ptr(out) + 4 * out_off,
                                   out_stride, npix, op, hip.stream()), "sisr_map64")


def _affine(t, g, shift, x, B, H, W, C):
    y = _empty_cl(B, C, H, W, t.device)
    hip.check(hip.lib().sisr_gate_residual_fwd(hip.ptr(t), hip.ptr(g), hip.ptr(shift), hip.ptr(x), hip.ptr(y), B,
                                               H * W, C, hip.stream()), "sisr_gate_residual_fwd")
    return y


def _pixel_sums(t, other, B, H, W, C=64):
    """[B][parts][C] ordered partial sums of t*other (other None: of t); C a multiple of 64."""
    L = hip.lib()
    parts = L.sisr_gate_dg_parts(H * W)
    part = torch.empty((B, parts, C), device=t.device, dtype=torch.float32)
    hip.check(L.sisr_gate_dg_partial(hip.ptr(t), hip.ptr(other), hip.ptr(part), B, H * W, C, hip.stream()),
              "sisr_gate_dg_partial")
    return part, parts


# ----------------------------------------------------------------------------- the families' public operators and constants
# (the modules import this one, so the block stands last)
from .convs import (conv_1x1, conv_f2y, conv_kxk, conv_kxk_s2, conv_s2_out_size, conv_y2f, convk_mfma,  # noqa: E402,F401
                    convk_mfma_leaky, pack_convk)
from .metrics import (MS_SSIM_MAX_LEVELS, MS_SSIM_WEIGHTS, ms_ssim_check_size, ms_ssim_min_side,  # noqa: E402,F401
                      ms_ssim_weights)
from .ops_attention import (SOCA_ITERS, SOCA_LIMIT, add_residual, ca_layer, conv3x3_stack, csam, gate_mul,  # noqa: E402,F401
                            global_avg_pool, lam, nonlocal_attention, nonlocal_block, pa_layer, pixel_shuffle, scale_add, soca,
                            soca_window, stack_maps)
from .ops_chain import FrozenChain, conv_chain, frozen_features, nchw_to_nhwc_pad, pad_param  # noqa: E402,F401
from .ops_dense import dense_block, dense_conv, dense_pack, dense_skip  # noqa: E402,F401
from .ops_losses import (SPECTRAL_MAX_SIDE, SPECTRAL_MIN_SIDE, SPECTRAL_TABLE_SLOTS, SSIM_WINDOW, degrade_valid,  # noqa: E402,F401
                         degrade_valid_tile, l1_loss, ms_ssim_mean, mse_loss, spectral_l1, spectral_tables, ssim_mean)
from .ops_sftmd import sft_apply, sft_layer, sftmd_forward  # noqa: E402,F401
from .ops_sparnet import (batch_norm_act, group_norm, instance_norm_act, leaky_relu, nearest_up, pixel_norm,  # noqa: E402,F401
                          prelu, refl_conv, selu, shuffle_rgb, spar_combine, spar_combine3d)
from .pool import map_mean  # noqa: E402,F401
