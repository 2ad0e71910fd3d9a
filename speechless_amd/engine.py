"""Device-side engine of the Wav2Letter hot path: owns HBM buffers (torch tensors = plumbing only) and sequences the
hand-written gfx950 kernels of libspeechless_hip.so for forward, CTC, backward, Adam.

Reference path being replaced (paths relative to the reference root): the Keras graph built by
speechless/net.py:291-341 (11 x Conv1D), :359-390 (loss_net, mean CTC loss, Adam 1e-4) and the two backend functions
:350-357 / :456-459.

HBM layout (see include/speechless_hip.h): every activation / gradient tensor is [B][HALO + Tt_pad + HALO][C_pad]
channels-last with zero halo rows, zero rows beyond the valid time and zero padded channels, so that a SAME-padded
conv tap is a row-shifted view.  The stride-2 first layer reads its input in the PAIR VIEW ([rows/2][2*C]).
Master weights / gradients / Adam moments live in ONE flat fp32 buffer each (layer order), in the Keras kernel layout
(k, Cin_pad, Cout_pad); the gradient buffer is what the data-parallel all-reduce operates on.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, launch_list
from ._lib import lib
from .buffers import _Buffers
from .engine_decode import DecodeAlignMixin, check_label_batch
from .engine_front import FrontLayerMixin
from .engine_launch import LaunchMixin, forward_epilogue, mask_epilogue
from .engine_split import SplitTopMixin
from .engine_x3 import X3Mixin
from ._hipevents import TimingEvent
from .plan import HALO, TIME_TILE, LayerPlan, LayerSpec, StackPlan, _round_up, same_padding, wav2letter_layer_specs  # noqa: F401


class Engine(StackPlan, LaunchMixin, X3Mixin, SplitTopMixin, FrontLayerMixin, DecodeAlignMixin):
    """Forward / CTC / backward / Adam on one MI355X.  dtype 'bf16' (bf16 storage, fp32 accumulate, fp32 CTC: the
    benchmarked path), 'f32' (parity path: fp32 storage, exact-fp32 MFMA) or 'bf16x3' (the fast parity path: every value as
    hi + lo bf16 planes, three bf16 MFMA terms per product, fp32 accumulate; csrc/split3.hip) or 'f16x3' (the same scheme on
    fp16 planes under power-of-two scales: w_scale, g_scale and, under a raw-wave front layer, x_scale)."""

    FRONT_DGRAD_ROW0 = 7          # first pair row of x0's gradient that is computed (frames start at pair row 11)
    FRONT_DGRAD_EXTRA_ROWS = 17   # pair rows computed beyond the output frames: up to row T' + 23 = the last frame's

    def __init__(self, specs, grapheme_set_size, dtype="bf16", device="cuda:0", ctc_epsilon=1e-8,
                 frozen_layer_count=0, lr=1e-4, beta_1=0.9, beta_2=0.999, adam_epsilon=1e-8, forward_only=False,
                 clipnorm=0.0, clipvalue=0.0, decay=0.0, track_grad_norm=False, criterion="ctc", optimizer="adam",
                 momentum=0.0, nesterov=False, rho=None):
        if criterion not in ("ctc", "asg"):
            raise ValueError("criterion must be 'ctc' or 'asg', not {!r}".format(criterion))
        if criterion == "asg" and (clipnorm or clipvalue or track_grad_norm):
            raise ValueError("criterion='asg': gradient clipping and the gradient norm cover the conv stack's flat gradient "
                             "buffer only, not the ASG tables -- clipnorm, clipvalue and track_grad_norm are not supported")
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("speechless_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                       "there is no CPU fallback for the hot path")
        self.lib = lib()
        self.device = torch.device(device)
        # the layout of the stack and the knobs its launch and bucket plans read (plan.py); complains about dtype and specs
        StackPlan.__init__(self, specs, grapheme_set_size, dtype, frozen_layer_count)
        if dtype == "bf16":
            self.torch_dtype, self.dtype_code = torch.bfloat16, _lib.SL_BF16
        elif dtype == "f32":
            self.torch_dtype, self.dtype_code = torch.float32, _lib.SL_F32
        elif dtype == "bf16x3":
            self.torch_dtype, self.dtype_code = torch.bfloat16, _lib.SL_BF16
        else:
            # f16x3: the plane scheme on fp16 pairs (round 6; engine_x3.py): 22 operand bits instead of 16-17 at the same three MFMA
            # terms.  fp16's range is 65504 and its precision below 2^-3 absolute, so weights and back-propagated gradients
            # are STORED multiplied by powers of two (exact) that bring typical magnitudes to ~1; the kernels divide them
            # out again (sl_conv_geom.acc_scale, the `scale` arguments of the sl_splitf16* helpers).
            self.torch_dtype, self.dtype_code = torch.float16, _lib.SL_F16
        self.x3_f16 = dtype == "f16x3"
        # f16x3: operand copies hold w_scale * w (glorot-uniform weights of this stack are 0.01 ... 0.05: x 64 -> ~1; representable
        # up to |w| < 1000), gradient planes hold g_scale * g (the CTC gradient of a frame is <= 1 / B: x 4096 stays below 2^12)
        self.w_scale = 64.0 if self.x3_f16 else 1.0
        self.g_scale = 4096.0 if self.x3_f16 else 1.0
        # f16x3 under a raw-wave front layer: the gathered sample windows hold x_scale * x (audio sits in [-1, 1] with quiet
        # passages orders of magnitude below; fp16 planes carry 22 bits only where |v| >= 2^-3: x 2^10 lifts samples down to
        # 2^-13 into that range and keeps full-scale audio a factor of 64 below 65504).  1 on every other path.
        self._x_scale = 1024.0 if (self.x3_f16 and self.front_spec is not None) else 1.0
        self.ctc_epsilon = ctc_epsilon
        self.lr, self.beta_1, self.beta_2, self.adam_epsilon = lr, beta_1, beta_2, adam_epsilon
        self.adam_iterations = 0
        # The update rule (Keras 2.0.x optimizers.py; include/speechless_hip.h "Keras-2.0 optimizers beside Adam"): "adam" (the
        # default: the sl_adam_* entry points with the arguments they always had), "sgd" (momentum, nesterov), "rmsprop" (rho),
        # "adagrad", "adadelta" (rho) or "adamax" (beta_1, beta_2).  `adam_epsilon` is every rule's epsilon.  The state buffers
        # keep their names: adam_m is the first slot of whatever rule runs, adam_v the second -- None for a one-slot rule,
        # which then moves 3 reads + 2 writes per parameter instead of 4 + 3.
        if optimizer not in _lib.OPT_RULES:
            raise ValueError("optimizer must be one of {}, not {!r}".format(", ".join(sorted(_lib.OPT_RULES)), optimizer))
        self.optimizer = optimizer
        self.opt_slots = _lib.OPT_SLOTS[optimizer]
        self.momentum, self.nesterov = float(momentum or 0.0), bool(nesterov)
        self.rho = float(rho) if rho is not None else (0.95 if optimizer == "adadelta" else 0.9)  # (Keras' defaults)
        # What every Keras 2.0 optimizer takes besides its own hyper-parameters (optimizers.py: Optimizer.get_gradients, the
        # `decay` of Adam.get_updates; include/speechless_hip.h "Gradient clipping on the device").  0 = off, and with all
        # three off the step launches exactly what it launched before they existed.
        #   clipnorm: the gradients of the trainable layers scaled by clipnorm / n when their global L2 norm n >= clipnorm --
        #     n is reduced on the device behind the last gradient of backward (sl_grad_sqnorm), the Adam launches read the
        #     factor from device memory: no host synchronisation, the recorded step replays it
        #   clipvalue: each element clamped to [-clipvalue, clipvalue] afterwards, inside the Adam kernels
        #   decay: lr = lr0 / (1 + decay * adam_iterations), on the host (adam_iterations is part of the optimizer state)
        # track_grad_norm: reduce n even without clipnorm (grad_norm).  The gradient buffer is never rewritten.
        self.clipnorm, self.clipvalue, self.decay = float(clipnorm or 0.0), float(clipvalue or 0.0), float(decay or 0.0)
        if self.clipnorm < 0 or self.clipvalue < 0 or self.decay < 0:
            raise ValueError("clipnorm, clipvalue and decay must be >= 0 (0 = off)")
        self.track_grad_norm = bool(track_grad_norm)
        self._norm_sq = self._norm_out = self._norm_ws = None  # device double; device floats (n, scale); partial sums
        self._norm_tables = {}
        dev = self.device
        off = self.param_numel
        self.params = torch.zeros((off,), dtype=torch.float32, device=dev)
        # forward_only: an evaluation engine (forward, CTC loss, decode) over masters another engine trains -- no gradient
        # buffer, no moments (Wav2Letter.eval_engine aliases `params` to the training engine's)
        self.forward_only = bool(forward_only)
        self.grads = self.adam_m = self.adam_v = None
        if not self.forward_only:
            self.grads = torch.zeros((off,), dtype=torch.float32, device=dev)
            self.adam_m = torch.zeros((off,), dtype=torch.float32, device=dev)
            if self.opt_slots == 2:
                self.adam_v = torch.zeros((off,), dtype=torch.float32, device=dev)
        # ASG criterion (csrc/asg.hip; DESIGN.md "ASG criterion"): the K x K transition scores g[from][to] and the K start
        # scores g0 are trainable parameters beside the conv stack's, in ONE flat fp32 buffer [g | g0] with a gradient and
        # Adam moments of the same shape -- one sl_adam_step launch updates both tables.  Zero = the paper's initialisation.
        self.criterion = criterion
        self.asg_params = self.asg_grads = self.asg_adam_m = self.asg_adam_v = None
        if criterion == "asg":
            if not 2 <= grapheme_set_size <= 64:
                raise ValueError("criterion='asg' takes 2 .. 64 graphemes (one lane per letter), not {}".format(grapheme_set_size))
            n_asg = _round_up(grapheme_set_size * (grapheme_set_size + 1), 4)  # (sl_adam_step works on groups of four)
            self.asg_params = torch.zeros((n_asg,), dtype=torch.float32, device=dev)
            if not self.forward_only:
                self.asg_grads, self.asg_adam_m, self.asg_adam_v = (
                    torch.zeros((n_asg,), dtype=torch.float32, device=dev) for _ in range(3))
                if self.opt_slots == 1:
                    self.asg_adam_v = None
        self._weights_set_count = 0
        pl = self.planes  # bf16x3: packed weight rows are [w_hi | w_hi | w_lo]
        self.w_fwd = [torch.zeros((p.cout_pad, p.spec.kernel_size, p.cin_pad * pl), dtype=self.torch_dtype, device=dev)
                      for p in self.all_plans]
        # (with a front layer the first layer of the stack needs its input gradient too: its dgrad operand in the pair view)
        self.w_dgrad = [torch.zeros((p.cin_pad, p.spec.kernel_size, p.cout_pad * pl), dtype=self.torch_dtype, device=dev)
                        if (0 < p.index < len(self.plans) or (p.index == 0 and self.front_plan is not None)) else None
                        for p in self.all_plans]
        self._packed_dirty = True
        self._buffers = {}
        self.max_cached_shapes = 4  # (batch, frames rounded up to 512) geometries kept allocated
        # Keras Dropout(rate) in front of every conv except the last three (net.py:301-303, 326-330); training steps
        # only.  None = off (every reference configuration).
        self.dropout_rate = None
        self.dropout_seed = 0
        self._dropout_steps = 0
        self.cur = None
        self._long_align = None  # buffers._AlignBuffers of ctc_align_long / asg_align_long, on first use
        self._long_viterbi = None  # buffers._AlignBuffers of asg_viterbi_long, on first use
        self._long_segment = None  # buffers._SegmentBuffers of ctc_ / asg_segment_scores_long, on first use
        self._long_spot = None  # buffers._SpotBuffers of ctc_spot_long, on first use
        self.timeline = None
        self.kernel_timeline = None  # (set of tags, list of (tag, start, stop)): see _around
        self._side_stream = None
        self._bgw_tables = {}
        self.fuse_output_softmax = os.environ.get("SL_FUSE_OUTPUT", "1") != "0"  # A/B knob: sl_output_softmax
        # both gradients of the 1x1 output layer in one launch that reads the layer's input once (sl_conv1d_backward_1x1):
        # 0.038 ms against 0.040 + 0.032 ms of dgrad + wgrad launches at config 3.  SL_FUSE_OUTPUT_BWD=0: the two launches.
        self.fuse_output_backward = os.environ.get("SL_FUSE_OUTPUT_BWD", "1") != "0"
        self.small_bias_pass_on_main = os.environ.get("SL_BIAS_MAIN", "1") != "0"  # A/B knob
        self.x3_fused_epilogue = os.environ.get("SL_X3_FUSED_EPILOGUE", "1") != "0"  # bf16x3: activation + plane split in the NT epilogue
        # bf16x3, striding layer: the g_lo partial of its weight gradient against the [hi0 | hi1] window of the pair rows
        # instead of the whole row (buffers.py; A/B knob, read when a buffer set's backward geometries are built)
        self.x3_b_window = os.environ.get("SL_X3_B_WINDOW", "1") != "0"
        # Launch lists (launch_list.py): the ~60 C-ABI calls and 4 stream hand-overs of a step are recorded the first time a
        # buffer set runs them and replayed afterwards with their arguments already marshalled -- the Python around each launch
        # (tensor views of the flat parameter buffers, data_ptr() calls, geometry look-ups: ~10 us per launch) was what
        # capped the host-fed loop below the rate of the resident step.  Geometries are passed by reference and
        # re-targeted in place (_Buffers.set_length), so one list serves every batch length of a buffer set.
        # runs of identical layers (inner_conv_1..7) as ONE launch with the activations kept in LDS (sl_conv1d_chain):
        # forward 124 us against 7 x 23.6 = 165 us of single launches, input gradients 126 against 185 (config 3;
        # HISTORY.md section 3.1).  SL_CHAIN=0 restores the single launches (A/B measurements).
        self.use_chain = os.environ.get("SL_CHAIN", "1") == "1"
        self.use_launch_lists = os.environ.get("SL_LAUNCH_LISTS", "1") != "0"
        if self.planes > 1:  # the fused launches read and write single-plane bf16 tensors (group_wgrad: plan.py)
            self.use_chain = self.fuse_output_softmax = self.fuse_output_backward = False
            self._x3_bias_ws = None
        # Split top: the CTC lattice is a handful of latency-bound waves (one per utterance and direction, T' sequential
        # frames: 0.106 ms at config 3, 0.39 ms at config 5) with the rest of the chip idle, and it sits between forward and
        # backward.  The training step therefore runs its TOP by half-batches: big_conv_1 / big_conv_2 / output_conv forward of
        # half A, then A's CTC on a side stream UNDER the same layers of half B; B's CTC under the input gradients of A's top
        # layers.  Per-utterance results do not depend on the half an utterance is in; weight gradients stay whole-batch
        # launches (sl_conv1d_backward_1x1_part accumulates the output layer's).  Used where it pays (_split_parts: long
        # utterances in small batches, i.e. configuration 5); SL_SPLIT_TOP=0: the whole-batch sequence everywhere.
        self.split_top = os.environ.get("SL_SPLIT_TOP", "1") != "0"
        if criterion == "asg":  # the split schedule launches the CTC of each part itself (engine_split.py): whole-batch sequence
            self.split_top = False
        self.split_min_tiles = None
        # Data-parallel runs: CUs the communication kernels are expected to own while a bucket is on the wire.  The MFMA
        # kernels take a whole CU per work-group and their grids are sized to whole rounds of the chip, so backward() tells
        # the library's choosers to plan for 256 - comm_cus (sl_set_available_cus) while an exchange can be in flight -- only
        # then: forward runs with the whole chip.  0 = no hint.  Set by train_step_resident from the reducer (comm_cus).
        self.comm_cus = 0
        self._cu_hint_active = 0  # what sl_set_available_cus was last told by this engine's backward (restored after sizing calls)
        self._ctc_streams = None
        self._rec = None
        self._adam_tables = {}
        self._sharded_reducer = None  # the reducer of the last step, if that step ran Adam on this rank's slices only

    # ------------------------------------------------------------------ plumbing

    @property
    def x_scale(self):
        """the power of two the gathered sample windows of the f16x3 raw-wave path are stored multiplied by (1024; 1 on every
        other path); the front layer's launches divide it out again.  Settable until the first batch is loaded."""
        return self._x_scale

    @x_scale.setter
    def x_scale(self, value):
        value = float(value)
        if not (self.x3_f16 and self.front_spec is not None):
            raise ValueError("x_scale belongs to the raw-wave front layer of an 'f16x3' engine")
        if not (0.0 < value < float("inf")) or np.frexp(value)[0] != 0.5:
            raise ValueError("x_scale must be a finite positive power of two, not {!r}".format(value))
        if self._buffers:
            raise ValueError("x_scale is fixed once the first batch is loaded (the buffer sets' geometries hold it)")
        self._x_scale = value

    def cu_hints(self):
        """the sl_set_available_cus settings this engine launches under (workspaces are sized for all of them)"""
        return [0, 256 - self.comm_cus] if self.comm_cus else [0]

    def set_comm_cus(self, comm_cus):
        """see self.comm_cus; re-sizes the split workspaces of the existing buffer sets for the new choosers' decisions"""
        comm_cus = int(comm_cus or 0)
        if comm_cus == self.comm_cus:
            return
        if comm_cus and not 0 < comm_cus <= 128:
            raise ValueError("comm_cus must be in 0 .. 128")
        self.comm_cus = comm_cus
        for buf in self._buffers.values():
            buf.invalidate()
            buf.size_nt_workspace(self, buf.fwd_geom, "fwd")
            if buf.bwd_ready:
                buf.size_backward_workspaces(self)

    @property
    def weights_version(self):
        """changes whenever the fp32 masters changed (set_weights, every optimizer step): what an engine sharing them compares"""
        return (self._weights_set_count, self.adam_iterations)

    def _set_cu_hint(self, cus):
        """sl_set_available_cus for the launches this THREAD enqueues from here on (the library keeps the setting per thread)
        and this engine's record of it -- one op of a recorded backward, so that a replayed step tracks it too and the sizing
        helpers that run in between (_max_over_cu_hints) restore the right value"""
        self.lib.call("sl_set_available_cus", cus)
        self._cu_hint_active = cus

    def _max_over_cu_hints(self, fn):
        """max of fn() under EVERY sl_set_available_cus setting this engine launches under -- the library's split choosers
        consult it, so a workspace sized under the data-parallel CU hint alone would be too small for a later step without it
         -- with the active setting restored whatever happens: it is process-wide library state"""
        need = 0
        try:
            for hint in self.cu_hints():
                self.lib.call("sl_set_available_cus", hint)
                need = max(need, fn())
        finally:
            self.lib.call("sl_set_available_cus", self._cu_hint_active)
        return need

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _launch(self, tag, name, *args):
        """One C-ABI call (tag = logical kernel instance, e.g. 'fwd:big_conv_1'): recorded while a launch list is being built,
        instrumented as a replayed launch would be while a measurement mode is on (_around)."""
        if self.timeline is None and self.kernel_timeline is None:
            self.lib.call(name, *args)
            if self._rec is not None:  # the raw entry point and its arguments
                self._rec.launch(self.lib.raw(name), args, name, tag, torch.cuda.current_stream(self.device))
            return
        rc = self._around()(self.lib.raw(name), args, tag, None)
        if rc != 0:
            launch_list.raise_status(name, rc, self.lib.last_error)

    def _around(self):
        """How a launch is instrumented right now (the `around` of launch_list.replay, and of _launch on the eager path), or
        None in the timed region.  self.timeline set (a list): HIP events on the launch stream around every call, for bench.py's
        per-launch table.  self.kernel_timeline set ((tags, list)): events attached to the main kernels of the tagged launches,
        for bench.py's roofline leg."""
        if self.timeline is not None:
            return launch_list.timed(self.timeline, TimingEvent)  # (timestamps only: no system-scope release between launches)
        if self.kernel_timeline is not None:
            return launch_list.profiled(
                *self.kernel_timeline, new_event=lambda: torch.cuda.Event(enable_timing=True),
                attach=lambda start, stop: self.lib.call("sl_profile_next_kernel", start.cuda_event, stop.cuda_event))
        return None

    def _hand_over(self, src, dst):
        """dst waits for everything enqueued on src so far (event record on src + wait on dst)."""
        ev = torch.cuda.Event()
        ev.record(src)
        dst.wait_event(ev)
        if self._rec is not None:
            self._rec.hand_over(ev, src, dst)

    def _bucket_ready(self, on_bucket_ready, b):
        """every launch that writes gradient bucket b is enqueued on the main stream"""
        on_bucket_ready(b)
        if self._rec is not None:
            self._rec.bucket_ready(b)

    def _eager_op(self, fn, *args):
        """fn(*args) now; while a launch list is being recorded it becomes ONE op of the list that calls fn again at
        replay (the launches inside are not recorded: their arguments change from batch to batch)"""
        rec, self._rec = self._rec, None
        try:
            fn(*args)
        finally:
            self._rec = rec
        if rec is not None:
            rec.eager(fn, args)

    def _run_recorded(self, buf, key, eager, callback=None):
        """One sequence of the step on buffer set `buf`: replays the launch list recorded under `key` (True), or runs eager()
        -- and keeps what it launches as that list unless a measurement mode instruments the launches, a list is already being
        recorded, or key is None (the sequence takes per-step values).  callback: on_bucket_ready of backward()."""
        usable = key is not None and self.use_launch_lists and self._rec is None
        ops = buf.launch_lists.get(key) if usable else None
        measuring = self.timeline is not None or self.kernel_timeline is not None
        if ops is not None:
            launch_list.replay(ops, callback, self._around() if measuring else None)
            return True
        if not usable or measuring:
            eager()
            return False
        self._rec = launch_list.Recorder(self.lib.last_error)
        try:
            eager()
            buf.launch_lists[key] = self._rec
        finally:
            self._rec = None
        return False

    def buffers(self, batch, t_in):
        """Buffers for batches of `batch` utterances padded to t_in frames: one set per (batch, output frames rounded
        up to TIME_TILE), re-targeted at t_in (see _Buffers.set_length)."""
        p0 = self.plans[0]
        t_out, _, _ = same_padding(t_in, p0.spec.kernel_size, p0.spec.stride)
        key = (batch, _round_up(max(t_out, 1), TIME_TILE))
        buf = self._buffers.get(key)
        if buf is None:
            if len(self._buffers) >= self.max_cached_shapes:  # bound HBM use when many batch shapes are seen
                self._buffers.pop(next(iter(self._buffers)))
            buf = _Buffers(self, batch, key[1])
            self._buffers[key] = buf
        buf.set_length(self, t_in)
        return buf

    def layer_param_views(self, tensor, plan):
        k = plan.spec.kernel_size
        w = tensor[plan.w_off: plan.w_off + plan.w_numel].view(k, plan.cin_pad, plan.cout_pad)
        b = tensor[plan.b_off: plan.b_off + plan.cout_pad]
        return w, b

    # ------------------------------------------------------------------ weights

    def _write_padded(self, flat, arrays, what):
        """arrays: [(W (k,Cin,Cout), b (Cout,))] numpy, Keras layout, into the padded flat buffer (zero everywhere else);
        what: the complaint about a layer (name, shapes) that does not fit"""
        flat.zero_()
        for p, (w, b) in zip(self._public_plans(), arrays):
            s = p.spec
            w = self._front_to_gemm(p, w)
            if tuple(w.shape) != (s.kernel_size, s.cin, s.cout) or tuple(b.shape) != (s.cout,):
                raise ValueError(what.format(s.name, w.shape, b.shape))
            wv, bv = self.layer_param_views(flat, p)
            wv[:, :s.cin, :s.cout] = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32)).to(self.device)
            bv[:s.cout] = torch.as_tensor(np.ascontiguousarray(b, dtype=np.float32)).to(self.device)

    def set_weights(self, weights):
        """weights: [(W (k,Cin,Cout), b (Cout,))] numpy, Keras layout."""
        assert len(weights) == len(self.all_plans)
        self._write_padded(self.params, weights, "weights of layer {} have shape {} / {}")
        for p in self.all_plans:
            if self._has_ones_output(p):  # relu(0 * x + 1) = elu(1) = 1: the ones channel (see self.ones_channel)
                self.layer_param_views(self.params, p)[1][p.cout_pad - 1] = 1.0
        self._packed_dirty = True
        self._weights_set_count += 1

    def _bias_grads_from_wgrad(self, layers, copy, stream):
        """One sl_bias_grad_from_wgrad launch for `layers` (their weight gradients are complete on `stream`)."""
        layers = list(layers)
        for lo in range(0, len(layers), 16):
            chunk = tuple(layers[lo:lo + 16])
            table = self._bgw_tables.get(chunk)
            if table is None:
                table = (_lib.BgwLayer * len(chunk))()
                for entry, i in zip(table, chunk):
                    q = self.plans[i]
                    entry.w_off, entry.b_off = q.w_off, q.b_off
                    entry.k, entry.cin_pad, entry.cout_pad, entry.tap = q.spec.kernel_size, q.cin_pad, q.cout_pad, q.pad_left
                self._bgw_tables[chunk] = table
            self._launch("bgrad_from_wgrad:{}..{}".format(self.plans[chunk[0]].spec.name, self.plans[chunk[-1]].spec.name),
                         "sl_bias_grad_from_wgrad", self.grads.data_ptr(), table, len(chunk), 1 if copy else 0,
                         stream.cuda_stream)

    def _unpad(self, tensor):
        out = []
        for p in self._public_plans():
            s = p.spec
            wv, bv = self.layer_param_views(tensor, p)
            out.append((self._front_from_gemm(p, wv[:, :s.cin, :s.cout].contiguous().cpu().numpy()),
                        bv[:s.cout].contiguous().cpu().numpy()))
        return out

    def get_weights(self):
        return self._unpad(self.params)

    def get_gradients(self):
        """The gradients of the last backward pass in the Keras layout.  (After a data-parallel step with a sharded
        optimizer only this rank's slice of every bucket holds the reduced gradient: reduce-scatter, not all-reduce.)"""
        return self._unpad(self.grads)

    def get_optimizer_state(self):
        """Adam moments in the Keras layout (per layer (m_W, m_b), (v_W, v_b)), the step count and the dropout step
        counter: everything beyond the weights that the next step depends on.
        After a step with a sharded optimizer (GradBucketReducer(shard_optimizer=True)) every rank holds the moments of its
        own slice of each bucket only: they are all-gathered here first, bucket by bucket with the slices of gather_bucket --
        a COLLECTIVE call in that case (every rank must make it; Wav2Letter.train does, each rank saves at the same epoch)."""
        reducer = self._sharded_reducer
        slots = self._state_slots()
        if reducer is not None and (reducer.world_size > 1 or reducer.force):
            for _, flat in slots:
                for b in range(len(reducer.ranges)):
                    reducer.gather_bucket(b, flat)
            reducer.wait_all()
        state = {name: self._unpad(flat) for name, flat in slots}
        state.update(iterations=int(self.adam_iterations), dropout_steps=int(self._dropout_steps))
        if self.optimizer != "adam":  # (an Adam state is the dictionary it always was; a state without the key is Adam)
            state["optimizer"] = self.optimizer
        return state

    def _state_slots(self):
        """the state buffers that exist, under the keys of the optimizer state: [("m", first slot)] or with ("v", second slot)"""
        return [("m", self.adam_m), ("v", self.adam_v)][:self.opt_slots]

    def set_optimizer_state(self, state):
        rule = str(state.get("optimizer", "adam"))
        if rule != self.optimizer:
            raise ValueError("the optimizer state is one of {!r}, this engine runs {!r}".format(rule, self.optimizer))
        for name, flat in self._state_slots():
            self._write_padded(flat, state[name], "optimizer state of layer {} has shape {} / {}")
        self.adam_iterations = int(state["iterations"])
        self._dropout_steps = int(state.get("dropout_steps", 0))

    def repack_weights(self):
        if self.planes > 1:
            return self._repack_weights_x3()
        st = self._stream()
        for p in self.all_plans:
            wv, _ = self.layer_param_views(self.params, p)
            wd = self.w_dgrad[p.index]
            k, cin = self._pack_dims(p)
            self._launch("pack:" + p.spec.name, "sl_pack_weights", wv.data_ptr(), self.w_fwd[p.index].data_ptr(),
                          wd.data_ptr() if wd is not None else None, k, cin, p.cout_pad, self.dtype_code, st)
        self._packed_dirty = False

    def _pack_dims(self, p):
        """(taps, input channels) the operand copies of plan p are packed with: the PAIR VIEW for a strided first layer that
        has a dgrad operand (same bytes for the forward operand; the flipped taps of the input-gradient operand are the
        pair view's 24, not the layer's 48)"""
        if p.index == 0 and p.spec.stride == 2 and self.w_dgrad[0] is not None and self.planes == 1:
            return p.taps_view, p.cin_view
        # (bf16x3: a frame's three planes sit side by side in a row, so the pair view of the FORWARD operand is the layer's
        # own (48, cin_pad) packing; the pair view of the input-gradient operand is packed apart, _pack_pair_dgrad_x3)
        return p.spec.kernel_size, p.cin_pad

    # ------------------------------------------------------------------ forward

    def load_input(self, input_batch):
        """input_batch: (B,T,F) numpy (any float dtype; the reference packs float64, net.py:583) or a float32 torch
        tensor already resident in HBM.  Raw-wave input on 'f16x3': the sample windows are stored as fp16 planes of
        x_scale * x, so samples must satisfy |x| * x_scale < 6.0e4 (|x| < 58 at the default 1024; audio sits in [-1, 1]) --
        beyond that the planes saturate at 65504.  Wav2Letter checks the host batches it packs; a device tensor is not read
        back here."""
        if isinstance(input_batch, np.ndarray):
            src = torch.from_numpy(np.ascontiguousarray(input_batch, dtype=np.float32)).to(self.device,
                                                                                            non_blocking=True)
        else:
            src = input_batch.to(device=self.device, dtype=torch.float32).contiguous()
        batch, t_in, f = src.shape
        if self.front_plan is not None:
            return self._load_front_input(src)
        if f != self.specs[0].cin:
            raise ValueError("input has {} bins per frame, the net expects {}".format(f, self.specs[0].cin))
        buf = self.buffers(batch, t_in)
        p0 = self.plans[0]
        if self.planes > 1:
            self._pack_input_x3(src, buf, t_in, f, self._stream())
        else:
            self._launch("pack_input", "sl_pack_input_ones", src.data_ptr(), buf.x0.data_ptr(), batch, t_in, f, p0.pad_left,
                         p0.cin_pad, buf.rows0 * p0.cin_pad, p0.cin_pad - 1 if self._has_ones_input() else -1, self.dtype_code,
                         self._stream())
        self.cur = buf
        self._src_keepalive = src
        return buf

    def _chain_table(self, kind, layers, buf):
        """ctypes pointer tables of sl_conv1d_chain for the given layers (plan indices in launch order), cached on the
        buffer set (freed with it).  kind 'fwd': ys = activations, ws = forward operands, biases; kind 'dgrad': layer i of the list
        is the input gradient of plan i: ys = g[i - 1], ws = dgrad operands, masks = y[i - 1]."""
        key = (kind, tuple(layers))
        hit = buf.chain_tables.get(key)
        if hit is not None:
            return hit
        n = len(layers)
        arr = ctypes.c_void_p * n
        if kind == "fwd":
            ys = arr(*[buf.y[i].data_ptr() for i in layers])
            ws = arr(*[self.w_fwd[i].data_ptr() for i in layers])
            aux = arr(*[self.layer_param_views(self.params, self.plans[i])[1].data_ptr() for i in layers])
        else:
            ys = arr(*[buf.g[i - 1].data_ptr() for i in layers])
            ws = arr(*[self.w_dgrad[i].data_ptr() for i in layers])
            aux = arr(*[buf.y[i - 1].data_ptr() for i in layers])
        buf.chain_tables[key] = (ys, ws, aux)
        return ys, ws, aux

    def _chain_ok(self, buf, layers):
        """the fused kernel takes a run of ReLU layers of the bf16 path whose geometry it supports"""
        if not self.use_chain or self.dtype != "bf16" or len(layers) < 2:
            return False
        if any(self.specs[i].activation != "relu" for i in layers):
            return False
        return bool(self.lib.raw("sl_conv1d_chain_supported")(ctypes.byref(buf.fwd_geom[layers[0]]), len(layers),
                                                              self.dtype_code))

    def forward(self, input_batch=None, training=False, split_ctc=None):
        """Runs the 11 conv layers + softmax.  Returns the probability tensor (B,T',K) fp32 in HBM.
        training=True applies dropout (if self.dropout_rate) to the inputs of the first n-3 layers: the packed input
        goes through sl_dropout into a second buffer, every other activation is dropped in place right after the
        layer that produced it (so the stored activation is the post-dropout one the backward pass needs).
        split_ctc=(grad_scale, a) (train_step_resident, a = split_top_plan()): the top three layers run in two parts of the
        batch -- utterances [0, a) and [a, B) -- and each part's CTC loss + gradient (ctc(grad_scale)) is launched on a side
        stream as soon as its probabilities exist; backward() picks the parts up (see self.split_top)."""
        if split_ctc is not None and self.criterion == "asg":
            raise ValueError("criterion='asg': the split-top schedule launches the CTC loss of each part; not supported")
        buf = self.load_input(input_batch) if input_batch is not None else self.cur
        if self._packed_dirty:
            self.repack_weights()
        st = self._stream()
        n = len(self.plans)
        rate = self.dropout_rate if training else None
        buf.dropped = bool(rate)
        buf.split_pending = 0
        if self.front_plan is not None and not rate and buf.front_frames_dropped:
            self._front_gather(buf, buf.front_src)  # (the last step gathered DROPPED samples; not part of any launch list)
        fuse_out = self.fuse_output_softmax and self.dtype == "bf16" and bool(self.lib.raw("sl_output_softmax_supported")(
            ctypes.byref(buf.fwd_geom[n - 1]), self.grapheme_set_size, self.dtype_code))
        # launch list (no dropout): everything below takes its frame count from the geometries, except the unfused
        # softmax, which gets it by value -> then the list is per length
        key = None if rate else ("fwd", st, fuse_out, self.use_chain, tuple(sorted(self.nt_cfg.items())),
                                 None if fuse_out else buf.t_out, split_ctc)
        if split_ctc is not None:
            # the part geometries (and the workspace they may re-allocate) exist BEFORE a list is looked up or recorded: a
            # launch of the lower layers already in the list being recorded would keep a freed nt_ws pointer
            self._presize_parts(buf, ("fwd", "dgrad") if buf.bwd_ready else ("fwd",), split_ctc[1])
        if self._run_recorded(buf, key, lambda: self._forward_eager(buf, rate, fuse_out, st, split_ctc)):
            buf.split_pending = split_ctc[1] if split_ctc is not None else 0
        return buf.probs

    def _forward_eager(self, buf, rate, fuse_out, st, split_ctc=None):
        if self.planes > 1:
            return self._forward_x3(buf, st, rate)
        n = len(self.plans)
        x, seed0 = self._forward_prologue(buf, rate, st)
        chained = {}  # first layer of a run -> the run, when it goes through sl_conv1d_chain
        if not rate:
            for (s0, e0) in self.runs:
                if e0 < n - 1 and self._chain_ok(buf, list(range(s0, e0 + 1))) and not any(
                        ("fwd", self.specs[i].name) in self.nt_cfg for i in range(s0, e0 + 1)):
                    chained[s0] = list(range(s0, e0 + 1))
        skip_until = -1
        for p in self.plans:
            last = p.index == n - 1
            if p.index <= skip_until:
                x = buf.y[p.index]
                continue
            if split_ctc is not None and p.index == n - 3:
                return self._forward_top_split(buf, x, st, split_ctc[0], split_ctc[1])
            if p.index in chained:
                layers = chained[p.index]
                ys, ws, biases = self._chain_table("fwd", layers, buf)
                self._launch("fwd:{}..{}".format(self.specs[layers[0]].name, self.specs[layers[-1]].name),
                             "sl_conv1d_chain", x.data_ptr(), ys, ws, biases, None, ctypes.byref(buf.fwd_geom[p.index]),
                             len(layers), _lib.EPI_BIAS_RELU, self.dtype_code, st)
                skip_until = layers[-1]
                x = buf.y[p.index]
                continue
            y = buf.logits if last else buf.y[p.index]
            _, bias = self.layer_param_views(self.params, p)
            if last and fuse_out:  # output layer + softmax + log(p + eps) re-normalisation in one launch
                self._launch("fwd:" + p.spec.name, "sl_output_softmax", x.data_ptr(), self.w_fwd[p.index].data_ptr(),
                             bias.data_ptr(), buf.probs.data_ptr(), buf.logq.data_ptr(), None,
                             ctypes.byref(buf.fwd_geom[p.index]), self.grapheme_set_size, p.cout_pad,
                             buf.tt_pad * p.cout_pad, self.ctc_epsilon, self.dtype_code, st)
                return buf.probs
            self._nt(buf, "fwd:" + p.spec.name, x, self.w_fwd[p.index], bias, None, y, buf.fwd_geom[p.index],
                     _lib.EPI_BIAS if last else forward_epilogue(p.spec.activation),
                     _lib.NT_OUT_F32 if last else _lib.NT_OUT_ELEM, self.nt_cfg.get(("fwd", p.spec.name), 0), st)
            if rate and (p.index + 1) in self._dropout_layers():
                self._launch("dropout:" + p.spec.name, "sl_dropout", y.data_ptr(), y.data_ptr(), y.numel(),
                             self.dtype_code, rate, seed0 + p.index + 1, st)
            x = y
        self._launch_softmax(buf, st)
        return buf.probs

    def set_input_lengths(self, prediction_lengths):
        buf = self.cur
        buf.input_len.copy_(torch.as_tensor(np.asarray(prediction_lengths, dtype=np.int32).reshape(-1)),
                            non_blocking=True)

    # ------------------------------------------------------------------ loss + backward

    def _check_label_width(self, width):
        """the CTC loss takes label batches of up to longform.CTC_LOSS_MAX_LABEL columns (the ASG loss states its own limit)"""
        from . import longform
        if self.criterion == "ctc" and width > longform.CTC_LOSS_MAX_LABEL:
            raise ValueError("label batch of {} columns: the CTC loss takes at most CTC_LOSS_MAX_LABEL = {} letters per label".format(
                int(width), longform.CTC_LOSS_MAX_LABEL))

    def set_labels(self, label_batch, label_lengths, prediction_lengths):
        """label_batch: int (B,Lmax) padded with anything (reference pads -1); lengths: (B,) or (B,1)."""
        buf = self.cur
        buf.ensure_backward(self)
        if np.ndim(label_batch) != 2 or np.shape(label_batch)[0] != buf.batch:
            raise ValueError("label batch must be (B, Lmax)")
        k = self.grapheme_set_size
        asg = self.criterion == "asg"  # (ASG has no blank: every index is a label)
        labels, lab_len = check_label_batch(label_batch, label_lengths, buf.batch, k if asg else k - 1,
                                            blank=None if asg else k - 1, check_lengths=False)
        self._check_label_width(labels.shape[1])
        l_max = max(int(labels.shape[1]), 1)
        if labels.shape[1] == 0:
            labels = np.zeros((buf.batch, 1), dtype=np.int32)
        buf.ensure_ctc(self, l_max)
        if buf.labels.shape[1] != labels.shape[1]:
            buf.labels = torch.zeros((buf.batch, labels.shape[1]), dtype=torch.int32, device=self.device)
        buf.labels.copy_(torch.from_numpy(np.ascontiguousarray(labels)), non_blocking=True)
        buf.label_len.copy_(torch.from_numpy(lab_len), non_blocking=True)
        self.set_input_lengths(prediction_lengths)

    def set_labels_resident(self, labels_dev, label_len_dev, input_len_dev):
        """set_labels for int32 tensors that already live in HBM (the staged input pipeline copies them on its copy
        stream): labels (B, Lmax >= 1) with every entry of row b below label_len[b] in [0, K-1), lengths (B,).  The
        tensors are used in place -- the caller keeps them alive and unchanged until the step's kernels have run."""
        buf = self.cur
        buf.ensure_backward(self)
        if labels_dev.dim() != 2 or labels_dev.shape[0] != buf.batch or labels_dev.shape[1] < 1:
            raise ValueError("label batch must be (B, Lmax >= 1)")
        self._check_label_width(labels_dev.shape[1])
        buf.ensure_ctc(self, int(labels_dev.shape[1]))
        buf.labels = labels_dev
        buf.label_len = label_len_dev
        buf.input_len = input_len_dev

    def _loss_grad_target(self, buf, grad_scale):
        """Where the criterion's kernel writes grad_scale * dL/dlogits -> (grad, halo, cp, batch_stride, code, scale): g[last]
        itself, or on the plane paths the fp32 staging buffer, whose rows are zeroed here (padded classes: the kernel writes
        the k real ones), under the planes' scale; _split_loss_grad then fills the planes of g[last] from it."""
        cp = self.plans[-1].cout_pad
        if self.planes > 1:
            buf.stage32[:buf.batch * buf.tt_pad * cp].zero_()
            return buf.stage32, 0, cp, buf.tt_pad * cp, _lib.SL_F32, grad_scale * self.g_scale
        return buf.g[-1], HALO, cp, buf.rows * cp, self.dtype_code, grad_scale

    def _split_loss_grad(self, buf, tag):
        """plane paths, behind the criterion's kernel: the staged fp32 gradient into the planes of g[last]"""
        cp = self.plans[-1].cout_pad
        self._split_planes(tag, buf.stage32, buf.g[-1], None, buf.batch, buf.t_out, cp, buf.tt_pad * cp, HALO,
                           buf.rows * cp * self.planes, _lib.SPLIT_COPY, self._stream())

    def ctc(self, grad_scale=None, with_grad=True):
        """Per-utterance CTC loss of the current probabilities (tensor (B,) in HBM) and, into g[last], the gradient
        w.r.t. the output_conv logits of grad_scale * sum_b loss_b (default 1/B: Keras' mean, net.py:389)."""
        buf = self.cur
        buf.ensure_backward(self)
        if grad_scale is None:
            grad_scale = 1.0 / buf.batch
        grad, halo, cp, batch_stride, code, scale = self._loss_grad_target(buf, grad_scale)
        self._launch("ctc", "sl_ctc_loss_grad", buf.probs.data_ptr(), buf.logq.data_ptr(), buf.labels.data_ptr(),
                     buf.label_len.data_ptr(), buf.input_len.data_ptr(), buf.loss.data_ptr(), grad.data_ptr(),
                     buf.batch, buf.t_out, self.grapheme_set_size, buf.labels.shape[1], halo, cp, batch_stride, code,
                     self.ctc_epsilon, scale, buf.ctc_ws.data_ptr(), buf.ctc_ws.numel(), self._stream())
        if self.planes > 1:
            self._split_loss_grad(buf, "split:ctc")
        return buf.loss

    # ------------------------------------------------------------------ ASG criterion (csrc/asg.hip)

    def _asg_views(self, flat):
        k = self.grapheme_set_size
        return flat[:k * k].view(k, k), flat[k * k:k * k + k]

    @property
    def asg_trans(self):
        """the transition scores g[from][to], float32 (K, K) in HBM (a view of asg_params)"""
        return self._asg_views(self.asg_params)[0]

    @property
    def asg_init(self):
        """the start scores g0, float32 (K,) in HBM (a view of asg_params)"""
        return self._asg_views(self.asg_params)[1]

    @property
    def asg_dtrans(self):
        return self._asg_views(self.asg_grads)[0]

    @property
    def asg_dinit(self):
        return self._asg_views(self.asg_grads)[1]

    def set_asg_scores(self, trans, init):
        """trans (K, K) [from][to] and init (K,) numpy: the scores themselves (not probabilities)"""
        k = self.grapheme_set_size
        trans, init = np.asarray(trans, dtype=np.float32), np.asarray(init, dtype=np.float32)
        if trans.shape != (k, k) or init.shape != (k,):
            raise ValueError("ASG scores must have shapes ({0}, {0}) and ({0},), not {1} and {2}".format(k, trans.shape, init.shape))
        self.asg_params[:k * k + k].copy_(torch.from_numpy(np.concatenate([trans.ravel(), init])))
        self._weights_set_count += 1

    def get_asg_state(self):
        """{'trans', 'init'} and, on a training engine, their Adam moments 'trans_m', 'trans_v', 'init_m', 'init_v' (numpy)"""
        out = {}
        named = [("", self.asg_params)] + ([] if self.forward_only else self._asg_state_slots())
        for suffix, flat in named:
            trans, init = self._asg_views(flat)
            out["trans" + suffix], out["init" + suffix] = trans.cpu().numpy().copy(), init.cpu().numpy().copy()
        return out

    def set_asg_state(self, state):
        """what get_asg_state returned (the moments are optional: a file of scores alone restarts them at zero)"""
        self.set_asg_scores(state["trans"], state["init"])
        if self.forward_only:
            return
        for suffix, flat in self._asg_state_slots():
            if "trans" + suffix in state:
                k = self.grapheme_set_size
                flat[:k * k + k].copy_(torch.from_numpy(np.concatenate([
                    np.asarray(state["trans" + suffix], dtype=np.float32).ravel(),
                    np.asarray(state["init" + suffix], dtype=np.float32).ravel()])))
            else:
                flat.zero_()

    def _asg_state_slots(self):
        return [("_m", self.asg_adam_m), ("_v", self.asg_adam_v)][:self.opt_slots]

    def _require_asg(self, what):
        if self.criterion != "asg":
            raise ValueError("{} needs an engine built with criterion='asg'".format(what))

    def asg(self, grad_scale=None):
        """ctc() for the ASG criterion: the per-utterance loss Z - N of the current probabilities under the engine's scores
        (tensor (B,) in HBM), into g[last] the gradient w.r.t. the output_conv logits of grad_scale * sum_b loss_b (default
        1/B), and into asg_dtrans / asg_dinit (overwritten) the gradients of the two tables.  A forward_only engine computes
        the loss alone.  Labels: set_labels, every index in [0, K)."""
        self._require_asg("asg()")
        buf = self.cur
        if grad_scale is None:
            grad_scale = 1.0 / buf.batch
        k = self.grapheme_set_size
        l_max = buf.labels.shape[1]
        buf.grow("asg_ws", self.lib.raw("sl_asg_workspace_bytes")(buf.batch, buf.tt_pad, k, l_max), 16)
        trans, init = self._asg_views(self.asg_params)
        ws = (buf.asg_ws.data_ptr(), buf.asg_ws.numel(), self._stream())
        if self.forward_only:
            self._launch("asg", "sl_asg_loss_grad", buf.probs.data_ptr(), buf.logq.data_ptr(), trans.data_ptr(), init.data_ptr(),
                         buf.labels.data_ptr(), buf.label_len.data_ptr(), buf.input_len.data_ptr(), buf.loss.data_ptr(), None,
                         None, None, buf.batch, buf.t_out, k, l_max, 0, k, 0, _lib.SL_F32, self.ctc_epsilon, grad_scale, *ws)
            return buf.loss
        buf.ensure_backward(self)
        grad, halo, cp, batch_stride, code, scale = self._loss_grad_target(buf, grad_scale)
        dtrans, dinit = self._asg_views(self.asg_grads)
        self._launch("asg", "sl_asg_loss_grad", buf.probs.data_ptr(), buf.logq.data_ptr(), trans.data_ptr(), init.data_ptr(),
                     buf.labels.data_ptr(), buf.label_len.data_ptr(), buf.input_len.data_ptr(), buf.loss.data_ptr(),
                     grad.data_ptr(), dtrans.data_ptr(), dinit.data_ptr(), buf.batch, buf.t_out, k, l_max, halo, cp,
                     batch_stride, code, self.ctc_epsilon, scale, *ws)
        if self.planes > 1:
            # (the table gradients carry the planes' power-of-two scale too: taken out again, exactly)
            if self.g_scale != 1.0:
                self._launch("scale:asg", "sl_scale", self.asg_grads.data_ptr(), self.asg_grads.numel(), _lib.SL_F32,
                             1.0 / self.g_scale, self._stream())
            self._split_loss_grad(buf, "split:asg")
        return buf.loss

    def loss(self, grad_scale=None):
        """the engine's criterion on the current probabilities and labels: ctc() or asg()"""
        return self.asg(grad_scale) if self.criterion == "asg" else self.ctc(grad_scale)

    def asg_adam_step(self):
        """Adam on the two ASG tables with the step's hyper-parameters and iteration count (adam_iterations already counts
        this step): one sl_adam_step launch over [g | g0].  Another rule: the same launch of its flat kernel."""
        self._launch_adam_flat("adam:asg", (self.asg_params, self.asg_grads, self.asg_adam_m, self.asg_adam_v), 0,
                               self.asg_params.numel(), self._stream(), clip=False)

    def backward(self, on_bucket_ready=None):
        """wgrad / bias-grad / dgrad for every trainable layer, output layer first.

        Bias gradients: layers whose input carries the ones channel get theirs out of the weight-gradient GEMM
        (_bias_grads_from_wgrad); the others (striding_conv; every layer when dropout touched the ones) by an HBM-bound
        sl_bias_grad pass over g[i] on a SIDE stream underneath the MFMA-bound wgrad / dgrad kernels.  Every hand-over to
        the side stream is an event record on the main stream and drains it for ~6 us (profiles/r01j: the only gaps of the
        step's timeline), and g[i] stays intact until the next step, so passes are collected until >= 128 MB of gradient
        are owed (or a bucket / the end of backward needs them).
        on_bucket_ready(b) is called once every launch that writes gradient bucket b (bucket_plan) is enqueued on the main
        stream -- the data-parallel reducer starts that bucket's exchange there."""
        buf = self.cur
        if self.forward_only:
            raise RuntimeError("this engine was built forward_only (evaluation): it has no gradient buffers")
        main = torch.cuda.current_stream(self.device)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)  # (ROCm offers no priority below the default)
        side = self._side_stream
        # launch list: not with dropout (its scale passes take the rate by value)
        key = None if buf.dropped else ("bwd", main.cuda_stream, buf.split_pending, on_bucket_ready is not None, self.ones_channel,
                                        self.frozen_layer_count, self.group_wgrad, self.use_chain, self.fuse_output_backward,
                                        self.use_wgrad_multi, self.multi_overlap_tiles, self.small_bias_pass_on_main,
                                        self.split_last_bucket, self.split_last_at,
                                        tuple(sorted(self.nt_cfg.items())),
                                        buf.t_out if self.planes > 1 else None)  # (bf16x3 helpers take it by value)
        try:
            norm = self._norm_wanted() and on_bucket_ready is None  # (data parallel: behind the exchange, train_step_resident)
            if norm:
                key = key and key + ("norm", self.clipnorm)
                self._norm_buffers(self._trainable_ranges())  # (allocated before a list keeps their pointers)

            def eager():
                self._backward_eager(buf, main, side, on_bucket_ready)
                if norm:  # every gradient is complete on the main stream here
                    self._launch_grad_norm(self._trainable_ranges(), main.cuda_stream)
            self._run_recorded(buf, key, eager, on_bucket_ready)
        except BaseException:
            if on_bucket_ready is not None and self.comm_cus:
                # raised between setting and clearing the CU hint: the library's setting is process-wide state shared by
                # every engine of the process -- do not leave it behind
                self._cu_hint_active = 0
                self.lib.raw("sl_set_available_cus")(0)
            raise

    def _dgrad_chains(self, buf, first):
        """input gradients of a run of identical ReLU layers in one launch (sl_conv1d_chain): {top layer: layers, top
        first}, and the set of layers such a launch covers besides its top layer"""
        dchain, skip = {}, set()
        if buf.dropped or not self.use_chain or self.dtype != "bf16":
            return dchain, skip
        cut = self._split_last_cut(first)
        for (s0, e0) in self.runs:
            layers = list(range(e0, max(s0, first + 1) - 1, -1))
            if len(layers) >= 2 and all(self.specs[i - 1].activation == "relu" for i in layers) and \
                    not any(("dgrad", self.specs[i].name) in self.nt_cfg for i in layers) and \
                    bool(self.lib.raw("sl_conv1d_chain_supported")(ctypes.byref(buf.dgrad_geom[e0]), len(layers),
                                                                   self.dtype_code)):
                pieces = [layers]
                if cut is not None and s0 < cut <= e0:
                    # split_last_bucket: input gradients of layers e0 .. cut first (they complete g[cut .. e0 - 1], all the
                    # upper weight-gradient launch still needs), the rest behind that launch
                    upper, lower = [i for i in layers if i >= cut], [i for i in layers if i < cut]
                    ok = all(len(q) == 1 or bool(self.lib.raw("sl_conv1d_chain_supported")(
                        ctypes.byref(buf.dgrad_geom[q[0]]), len(q), self.dtype_code)) for q in (upper, lower) if q)
                    if ok:
                        pieces = [q for q in (upper, lower) if q]
                for q in pieces:
                    if len(q) >= 2:
                        dchain[q[0]] = q
                        skip.update(q[1:])
        return dchain, skip

    def _launch_wgrad(self, buf, i, grouped, st):
        """weight gradient of layer i -- or, at the lowest layer of a grouped run, of the whole run"""
        p = self.plans[i]
        if i in grouped:
            lo, hi = grouped[i]
            if i != lo:
                return  # every g[lo..hi] is complete only at the lowest layer: one launch for the run there
            plo = self.plans[lo]
            dw_lo, _ = self.layer_param_views(self.grads, plo)
            stride_elems = buf.batch * buf.rows * plo.cin_pad
            self._launch("wgrad:{}..{}".format(plo.spec.name, self.plans[hi].spec.name), "sl_conv1d_wgrad_grouped",
                         buf.y[lo - 1].data_ptr(), buf.g[lo].data_ptr(), dw_lo.data_ptr(),
                         ctypes.byref(buf.wgrad_geom[lo]), hi - lo + 1, stride_elems, stride_elems,
                         plo.w_numel + plo.cout_pad, 0, buf.wgrad_ws.data_ptr(), buf.wgrad_ws.numel(), st)
            return
        x = (buf.x0_dropped if buf.dropped else buf.x0) if i == 0 else buf.y[i - 1]
        dw, _ = self.layer_param_views(self.grads, p)
        self._wgrad(buf, "wgrad:" + p.spec.name, x, buf.g[i], dw, buf.wgrad_geom[i],
                    self.nt_cfg.get(("wgrad", p.spec.name), 0), st)

    def _fused_output_backward(self, buf, i, first, grouped, dchain, dchain_skip):
        """layer i's weight AND input gradient in one sl_conv1d_backward_1x1 launch: the 1x1 output layer on the bf16 path"""
        if not self.fuse_output_backward or i != len(self.plans) - 1 or i <= first or self.dtype != "bf16":
            return False
        if i in grouped or i in dchain or i in dchain_skip or buf.bwd1x1_ws is None:
            return False
        name = self.specs[i].name
        if ("wgrad", name) in self.nt_cfg or ("dgrad", name) in self.nt_cfg:
            return False
        if self.specs[i - 1].activation not in ("relu", "elu") or (buf.dropped and i in self._dropout_layers()):
            return False
        return bool(self.lib.raw("sl_conv1d_backward_1x1_supported")(ctypes.byref(buf.wgrad_geom[i]),
                                                                     self.grapheme_set_size, self.dtype_code))

    def _launch_output_backward(self, buf, i, st):
        p = self.plans[i]
        dw, _ = self.layer_param_views(self.grads, p)
        self._launch("bwd:" + p.spec.name, "sl_conv1d_backward_1x1", buf.y[i - 1].data_ptr(), buf.g[i].data_ptr(),
                     self.w_dgrad[i].data_ptr(), buf.g[i - 1].data_ptr(), dw.data_ptr(), ctypes.byref(buf.wgrad_geom[i]),
                     mask_epilogue(self.specs[i - 1].activation), self.grapheme_set_size, self.dtype_code, 0,
                     buf.bwd1x1_ws.data_ptr(), buf.bwd1x1_ws.numel(), st)

    def _launch_dgrad(self, buf, i, st):
        """input gradient of layer i into g[i - 1], through the activation of layer i - 1 (and its dropout)"""
        name = self.specs[i].name
        self._dgrad_through(buf, name, buf.g[i], self.w_dgrad[i], buf.y[i - 1], buf.g[i - 1], buf.dgrad_geom[i],
                            self.specs[i - 1].activation, buf.dropped and i in self._dropout_layers(), buf.dropout_seed0 + i,
                            self.nt_cfg.get(("dgrad", name), 0), st)

    def _wgrad_multi_workspace_need(self, table, n_jobs):
        """workspace of a balanced weight-gradient launch: its segment count is 2 * CUs / tiles (_max_over_cu_hints)"""
        return self._max_over_cu_hints(
            lambda: self.lib.raw("sl_conv1d_wgrad_multi_workspace_bytes")(table, n_jobs, self.dtype_code))

    def _wgrad_multi_table(self, buf, layers):
        """job table of a balanced weight-gradient launch over `layers`, built once per buffer set; makes sure the shared
        workspace covers it.  backward() builds the tables of ALL its balanced launches before the first of them is enqueued:
        a workspace re-allocated for the second launch would leave the first one's recorded launch with a freed pointer."""
        key = (tuple(layers), buf.dropped)
        table = buf.multi_tables.get(key)
        if table is None:
            table = (_lib.WgradJob * len(layers))()
            for job, i in zip(table, layers):
                x = (buf.x0_dropped if buf.dropped else buf.x0) if i == 0 else buf.y[i - 1]
                dw, _ = self.layer_param_views(self.grads, self.plans[i])
                job.x, job.g, job.dw = x.data_ptr(), buf.g[i].data_ptr(), dw.data_ptr()
                job.geom.copy_from(buf.wgrad_geom[i])
            buf.multi_tables[key] = table
            buf.grow("wgrad_multi_ws", self._wgrad_multi_workspace_need(table, len(layers)), 16, first_drops=False)
        return table

    def _launch_wgrad_multi(self, buf, layers, st):
        table = self._wgrad_multi_table(buf, layers)
        self._launch("wgrad:{}..{}".format(self.specs[layers[0]].name, self.specs[layers[-1]].name),
                     "sl_conv1d_wgrad_multi", table, len(layers), self.dtype_code, buf.wgrad_multi_ws.data_ptr(),
                     buf.wgrad_multi_ws.numel(), st)

    def _backward_eager(self, buf, main, side, on_bucket_ready):
        if self.planes > 1:
            return self._backward_x3(buf, main.cuda_stream, on_bucket_ready)
        first = self.frozen_layer_count
        grouped = self._grouped_wgrad_runs(first)
        dchain, dchain_skip = self._dgrad_chains(buf, first)
        multi = {}  # layer -> the layers of the balanced launch that writes its weight gradient (at the lowest of them)
        for launch_layers in self._wgrad_multi_groups(first, grouped):
            self._wgrad_multi_table(buf, launch_layers)
            for i in launch_layers:
                multi[i] = launch_layers
        # bias gradients out of the weight-gradient GEMM (self.ones_channel): which layers, and whether the row holds the
        # bias gradient (the ones were not touched by dropout) or only has to be zeroed before the optimizer sees it
        ones_in = self._ones_input_layers(first)
        ones_db = set() if buf.dropped else set(ones_in)
        # data parallel: bucket b is complete once the weight gradient of its LOWEST layer is enqueued
        plan = self.bucket_plan() if on_bucket_ready is not None else []
        bucket_at = {layers[0]: (b, layers) for b, (layers, _) in enumerate(plan)}
        side_busy = [False]

        def flush_bias_passes(pending):
            """sl_bias_grad passes of the layers in `pending` (their g is complete at this point of MAIN) on SIDE -- a lone
            small pass (the first layer's 8 MB, the only one left beside the ones channel) on MAIN: two hand-overs cost the
            main stream 6.5 us each (rocprof timeline), the pass itself 9"""
            def bias_pass(j, stream):
                _, db_j = self.layer_param_views(self.grads, self.plans[j])
                self._launch("bgrad:" + self.plans[j].spec.name, "sl_bias_grad", buf.g[j].data_ptr(), db_j.data_ptr(),
                             ctypes.byref(buf.wgrad_geom[j]), self.dtype_code, buf.bias_ws.data_ptr(),
                             buf.bias_ws.numel(), stream.cuda_stream)

            if len(pending) == 1 and buf.g[pending[0]].numel() * buf.g[pending[0]].element_size() <= (32 << 20) \
                    and self.small_bias_pass_on_main:
                bias_pass(pending[0], main)
                del pending[:]
                return
            self._hand_over(main, side)
            with torch.cuda.stream(side):
                for j in pending:
                    bias_pass(j, side)
            side_busy[0] = True
            del pending[:]

        def join_side():
            if side_busy[0]:
                self._hand_over(side, main)
                side_busy[0] = False

        n = len(self.plans)
        split = buf.split_pending
        if split:  # the CTC ran in two parts: so do the input gradients of the top three layers (see self.split_top)
            self._backward_top_split(buf, main, split)
        pending, pending_bytes = [], 0  # layers whose bias-gradient pass is still owed to the side stream
        for p in reversed(self.plans[first:]):
            i = p.index
            if i not in ones_db:
                pending.append(i)
                pending_bytes += buf.g[i].numel() * buf.g[i].element_size()
            closes_bucket = i in bucket_at
            if pending and (pending_bytes >= (128 << 20) or i == first or closes_bucket):
                flush_bias_passes(pending)
                pending_bytes = 0
            fused_bwd = self._fused_output_backward(buf, i, first, grouped, dchain, dchain_skip)
            if split and i == n - 1:
                pass  # weight + input gradient of the output layer: done by halves above
            elif fused_bwd:
                self._launch_output_backward(buf, i, main.cuda_stream)
            elif i in multi:
                if i == multi[i][0]:  # every gradient tensor the launch reads is complete at its lowest layer
                    self._launch_wgrad_multi(buf, multi[i], main.cuda_stream)
            else:
                self._launch_wgrad(buf, i, grouped, main.cuda_stream)
            if closes_bucket:
                self._close_bucket(on_bucket_ready, *bucket_at[i], ones_in, ones_db, main, join_side)
            if i in dchain:
                layers = dchain[i]
                ys, ws, masks = self._chain_table("dgrad", layers, buf)
                self._launch("dgrad:{}..{}".format(self.specs[layers[0]].name, self.specs[layers[-1]].name),
                             "sl_conv1d_chain", buf.g[i].data_ptr(), ys, ws, None, masks,
                             ctypes.byref(buf.dgrad_geom[i]), len(layers), _lib.EPI_RELU_MASK, self.dtype_code,
                             main.cuda_stream)
            elif i > first and i not in dchain_skip and not fused_bwd and not (split and i >= n - 3):
                self._launch_dgrad(buf, i, main.cuda_stream)
        self._backward_tail(buf, on_bucket_ready, ones_in, ones_db, main, join_side)

    def adam_step(self, fused=True):
        """Keras-2.0 Adam on the flat fp32 masters.  fused=True: one kernel per trainable layer that applies Adam AND
        rewrites the layer's two bf16 operand copies in the same pass (no separate repack); fused=False: one flat
        elementwise launch, operands repacked lazily by the next forward()."""
        if self.forward_only:
            raise RuntimeError("this engine was built forward_only (evaluation): it has no optimizer state")
        self.adam_iterations += 1
        st = self._stream()
        if not fused:
            self._launch_adam_flat("adam", self._state_buffers(), 0, self.param_numel, st)
            self._packed_dirty = True
            return
        if self._packed_dirty:
            self.repack_weights()  # frozen layers keep these copies; trainable ones are rewritten below
        self._adam_layers(self._trainable_layers(), st)

    def _lr_now(self):
        """the learning rate of the update being launched (self.adam_iterations already counts it): Keras 2.0 Adam's
        lr * 1 / (1 + decay * iterations) with iterations = the updates completed before this one"""
        if not self.decay:
            return self.lr
        return self.lr * (1.0 / (1.0 + self.decay * (self.adam_iterations - 1)))

    def _clip_args(self):
        """(grad_scale device pointer or None, clipvalue) of the clipped Adam twins, or None: launch the originals"""
        if not (self.clipnorm > 0 or self.clipvalue > 0):
            return None
        return (self._norm_out[1:].data_ptr() if self.clipnorm > 0 else None, self.clipvalue)

    def _opt_rule(self):
        """sl_opt_rule of the update being launched (a rule beside Adam; self.adam_iterations already counts it): the decayed
        rate -- Adamax: divided by 1 - beta_1^t here, in double -- and the rule's coefficients"""
        rule = _lib.OptRule()
        rule.rule = _lib.OPT_RULES[self.optimizer]
        lr = self._lr_now()
        if self.optimizer == "adamax":
            lr = lr / (1.0 - self.beta_1 ** self.adam_iterations)
        rule.lr, rule.momentum, rule.nesterov, rule.rho = lr, self.momentum, int(self.nesterov), self.rho
        rule.beta1, rule.beta2, rule.eps = self.beta_1, self.beta_2, self.adam_epsilon
        return rule

    def _state_buffers(self):
        return (self.params, self.grads, self.adam_m, self.adam_v)

    def _launch_update(self, tag, name, what, pre, post, st, clip=True):
        """One launch of the update, flat or fused: the ONE place that tells Adam from the other rules.  tag and name are Adam's
        ('adam...', 'sl_*adam_*'); another rule launches the same kernel family as 'opt:<rule>...' / 'opt_shard:<rule>...' through
        'sl_*optimizer_*' with an sl_opt_rule where Adam passes (step, lr, beta_1, beta_2, epsilon).  Clipping: Adam's clipped twin
        when there is any, else the original entry point with the arguments it always had; the other rules' entry points take
        (None, 0) for none.  pre / post: the operand format's arguments in front of / behind the coefficients."""
        clip = self._clip_args() if clip else None
        if self.optimizer == "adam":
            how = (self.adam_iterations, self._lr_now(), self.beta_1, self.beta_2, self.adam_epsilon)
            name, clip = (name, ()) if clip is None else (name + "_clipped", clip)
        else:
            kind, _, rest = tag.partition(":")
            tag = "{}:{}{}".format(kind.replace("adam", "opt"), self.optimizer, ":" + rest if rest else "")
            name, how, clip = name.replace("adam", "optimizer"), (self._opt_rule(),), clip or (None, 0.0)
        self._launch(tag, name, *what, *pre, *how, *post, *clip, st)

    def _launch_adam_flat(self, tag, buffers, lo, hi, st, clip=True):
        """plain elementwise update on [lo, hi) of `buffers` = (parameters, gradients, first and second state slot: None for a
        one-slot rule): the unfused step, a rank's slice under the sharded optimizer, the ASG tables (clip=False).
        tag: 'adam' / 'adam_shard:<b>' / 'adam:asg'"""
        what = [t[lo:hi].data_ptr() if t is not None else None for t in buffers]
        self._launch_update(tag, "sl_adam_step", (*what, hi - lo), (), (), st, clip)

    # ------------------------------------------------------------------ gradient norm (clipnorm, track_grad_norm)

    def _norm_wanted(self):
        return (self.clipnorm > 0 or self.track_grad_norm) and not self.forward_only

    @property
    def grad_norm(self):
        """0-d device tensor (fp32, not synchronised): the global L2 norm of the trainable layers' gradients of the last
        backward pass / step, before any clipping; None unless clipnorm > 0 or track_grad_norm"""
        if not self._norm_wanted():
            return None
        self._norm_buffers(self._trainable_ranges())
        return self._norm_out[0]

    def _norm_table(self, ranges):
        key = tuple(ranges)
        table = self._norm_tables.get(key)
        if table is None:
            if not 1 <= len(key) <= 16:
                raise ValueError("the gradient norm takes 1 .. 16 ranges per launch")
            table = (_lib.NormRange * len(key))()
            for entry, (lo, hi) in zip(table, key):
                entry.offset, entry.count = lo, hi - lo
            self._norm_tables[key] = table
        return table

    def _norm_buffers(self, ranges):
        """the device scalars (allocated once: recorded launches keep their pointers) and a workspace that covers `ranges`"""
        if self._norm_sq is None:
            self._norm_sq = torch.zeros((1,), dtype=torch.float64, device=self.device)
            self._norm_out = torch.zeros((2,), dtype=torch.float32, device=self.device)  # n, clip factor
            self._norm_out[1] = 1.0
        table = self._norm_table(ranges)
        need = self.lib.raw("sl_grad_sqnorm_workspace_bytes")(table, len(table))
        if self._norm_ws is None or self._norm_ws.numel() * 8 < need:
            self._norm_ws = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=self.device)
            for buf in self._buffers.values():
                buf.launch_lists.clear()  # (recorded backward lists hold the old workspace pointer)
        return table

    def _launch_grad_norm(self, ranges, st, finish=True):
        """sum of g * g over `ranges` of the gradient buffer into the device double; finish: also n and the clip factor (one
        process holds the whole gradient) -- else the caller all-reduces the double and calls _launch_clip_scale"""
        table = self._norm_buffers(ranges)
        out = self._norm_out
        self._launch("grad_norm", "sl_grad_sqnorm", self.grads.data_ptr(), table, len(table), self.clipnorm,
                     self._norm_sq.data_ptr(), out.data_ptr() if finish else None, out[1:].data_ptr() if finish else None,
                     self._norm_ws.data_ptr(), self._norm_ws.numel() * 8, st)

    def _launch_clip_scale(self, st):
        self._launch("clip_scale", "sl_clip_scale", self._norm_sq.data_ptr(), 1, self.clipnorm, self._norm_out[1:].data_ptr(),
                     self._norm_out.data_ptr(), st)

    def _adam_table(self, chunk):
        table = self._adam_tables.get(tuple(chunk))
        if table is None:  # (the operand copies never move: built once per set of layers)
            table = (_lib.AdamLayer * len(chunk))()
            for entry, i in zip(table, chunk):
                p = self.all_plans[i]
                wd = self.w_dgrad[p.index]
                if self.planes > 1 and p.index == 0 and p is not self.front_plan:
                    wd = None  # bf16x3 under a raw-wave front layer: _pack_pair_dgrad_x3 rewrites this operand
                entry.offset = p.w_off
                entry.w_fwd = self.w_fwd[p.index].data_ptr()
                entry.w_dgrad = wd.data_ptr() if wd is not None else None
                entry.k, entry.cin_pad = self._pack_dims(p)
                entry.cout_pad = p.cout_pad
            self._adam_tables[tuple(chunk)] = table
        return table

    def _adam_layers(self, layers, st):
        """Fused update + operand repack of the given layers on stream st (self.adam_iterations already counts this step):
        ONE launch for all of them (sl_*adam_pack_layers; another rule: sl_*optimizer_pack_layers), 16 layers per call at
        most."""
        # per operand format: the entry point and its arguments in front of / behind the rule's coefficients
        # (bf16x3: the [w_hi | w_hi | w_lo] operand rows are rewritten in the same pass, layer 0's pair view behind it)
        if self.planes == 3:
            name, scaled = self._plane_entry("sl_split3_adam_pack_layers")
            pre, post, pair = (), (self.w_scale,) if scaled else (), self.w_dgrad[0] is not None
        else:
            name, pre, post, pair = "sl_adam_pack_layers", (self.dtype_code,), (), False
        layers = list(layers)
        for lo in range(0, len(layers), 16):
            chunk = layers[lo:lo + 16]
            tag = "adam:{}..{}".format(self.all_plans[chunk[0]].spec.name, self.all_plans[chunk[-1]].spec.name)
            what = [t.data_ptr() if t is not None else None for t in self._state_buffers()]
            self._launch_update(tag, name, (*what, self._adam_table(chunk), len(chunk)), pre, post, st)
            if pair and 0 in chunk:
                self._pack_pair_dgrad_x3(st)

    def train_step(self, input_batch, label_batch, label_lengths, prediction_lengths, reducer=None):
        """One full optimisation step (forward, CTC, backward, [gradient all-reduce], Adam, weight repack).
        Returns the per-utterance loss tensor (B,) in HBM (not synchronised)."""
        self.load_input(input_batch)
        self.set_labels(label_batch, label_lengths, prediction_lengths)
        return self.train_step_resident(reducer)

    def train_step_resident(self, reducer=None):
        """Same, with input / labels / lengths already resident in HBM (bench.py's timed region)."""
        dp = reducer is not None and (reducer.world_size > 1 or reducer.force)
        if dp and self.criterion == "asg":
            raise ValueError("criterion='asg': the gradients of the ASG tables are in no bucket of the data-parallel exchange; "
                             "train on one GPU")
        world = reducer.world_size if reducer is not None else 1
        self._sharded_reducer = reducer if (dp and reducer.shard_optimizer) else None
        self.set_comm_cus(getattr(reducer, "comm_cus", 0) if dp else 0)
        grad_scale = 1.0 / (self.cur.batch * world)
        part = self.split_top_plan(self.cur)
        if part:
            self.forward(training=True, split_ctc=(grad_scale, part))  # ... and the CTC, in two parts (self.split_top)
            loss = self.cur.loss
        else:
            self.forward(training=True)
            loss = self.loss(grad_scale=grad_scale)
        if not dp:
            self.backward()
            self.adam_step()
            if self.criterion == "asg":
                self.asg_adam_step()
            return loss
        self.backward(on_bucket_ready=reducer.reduce_bucket)
        # every bucket's exchange was started the moment its last weight gradient was enqueued; the big ones finished
        # under the rest of backward.  Update bucket by bucket, in the order the exchanges complete.
        if self._packed_dirty:
            self.repack_weights()
        self.adam_iterations += 1
        st = self._stream()
        plan = self.bucket_plan()
        if self._norm_wanted():
            # the norm needs every reduced gradient before any layer is updated: wait for ALL buckets here (the bucket-by-bucket
            # overlap of exchange and update below is given up; the waits below find nothing outstanding)
            reducer.wait_all()
            if not reducer.shard_optimizer:  # every rank reduces the same reduced buffer in the same order: the same bits
                self._launch_grad_norm(self._trainable_ranges(), st)  # (= the buckets' layers, in the single process's order)
            else:  # this rank's slices, then ONE scalar all-reduce (sum, double) through the reducer's process group
                self._launch_grad_norm([reducer.shard_of(lo, hi) for _, (lo, hi) in plan], st, finish=False)
                reducer.all_reduce_scalar(self._norm_sq)
                self._launch_clip_scale(st)
        if not reducer.shard_optimizer:
            for layers, _ in plan:
                reducer.wait_next()
                self._adam_layers(layers, st)
            return loss
        # sharded optimizer: each bucket was reduce-SCATTERED; this rank holds the summed gradient of its 1/world slice
        # only, updates that slice (plain elementwise Adam, 1/world of the optimizer's HBM traffic), and the updated
        # fp32 masters are all-gathered in place; the operand copies are rewritten from the gathered masters
        for b, (layers, (lo, hi)) in enumerate(plan):
            reducer.wait_next()
            slo, shi = reducer.shard_of(lo, hi)
            self._launch_adam_flat("adam_shard:{}".format(b), self._state_buffers(), slo, shi, st)
            reducer.gather_bucket(b, self.params)
        for layers, _ in plan:
            reducer.wait_next()
            self._pack_layers(layers, st)
        return loss

    def _pack_layers(self, layers, st):
        """both operand copies of the given layers rewritten from the fp32 masters: one launch (sl_pack_layers)"""
        if self.planes == 3:  # bf16x3: one launch per layer
            for i in layers:
                p = self.all_plans[i]
                wv, _ = self.layer_param_views(self.params, p)
                wd = self.w_dgrad[p.index]
                pair = wd is not None and p.index == 0 and p is not self.front_plan  # (its pair view: _pack_pair_dgrad_x3)
                self._pack_weights_x3("pack3:" + p.spec.name, wv, self.w_fwd[p.index], wd if (wd is not None and not pair) else None,
                                      p.spec.kernel_size, p.cin_pad, p.cout_pad, st)
                if pair:
                    self._pack_pair_dgrad_x3(st)
            return
        layers = list(layers)
        for lo in range(0, len(layers), 16):
            chunk = layers[lo:lo + 16]
            self._launch("pack:{}..{}".format(self.all_plans[chunk[0]].spec.name, self.all_plans[chunk[-1]].spec.name),
                         "sl_pack_layers", self.params.data_ptr(), self._adam_table(chunk), len(chunk), self.dtype_code,
                         st)
