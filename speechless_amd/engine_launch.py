"""The engine's launch helpers: each is the ONE place that spells out the argument list of its C-ABI entry point, the plane
helpers the one place that knows a plane entry point's fp16 twin; on top of them the layer steps and the frame (prologue,
softmax, bucket close, tail) that the single-plane and the plane loops share.  Methods of Engine."""
import ctypes

import torch

from . import _lib

# plane entry point on bf16 pairs -> (its twin on fp16 pairs, the twin takes a power-of-two scale behind the shared arguments)
F16_TWINS = {
    "sl_split3": ("sl_splitf16", False),
    "sl_split3_pack_input": ("sl_splitf16_pack_input", False),
    "sl_split3_dropout": ("sl_splitf16_dropout", False),
    "sl_split3_pack_weights": ("sl_splitf16_pack_weights", True),
    "sl_split3_bias_grad": ("sl_splitf16_bias_grad", True),
    "sl_split3_wgrad_combine": ("sl_split3_wgrad_combine_scaled", True),
    "sl_split3_adam_pack_layers": ("sl_splitf16_adam_pack_layers", True),
}


def _ptr(operand):
    """an operand of a launch: a tensor (its address), None, or an address (engine_split.py: an utterance inside a tensor)"""
    return operand.data_ptr() if isinstance(operand, torch.Tensor) else operand


def forward_epilogue(activation):
    return _lib.EPI_BIAS_ELU if activation == "elu" else _lib.EPI_BIAS_RELU


def mask_epilogue(activation):
    return _lib.EPI_ELU_MASK if activation == "elu" else _lib.EPI_RELU_MASK


class LaunchMixin:
    # ------------------------------------------------------------------ entry points
    def _nt(self, buf, tag, x, w, bias, mask, out, geom, epi, out_mode, cfg, st):
        self._launch(tag, "sl_conv1d_nt", _ptr(x), _ptr(w), _ptr(bias), _ptr(mask), _ptr(out), ctypes.byref(geom), epi,
                     self.dtype_code, out_mode, cfg, buf.nt_ws.data_ptr(), buf.nt_ws.numel(), st)

    def _wgrad(self, buf, tag, x, g, dw, geom, cfg, st):
        self._launch(tag, "sl_conv1d_wgrad", _ptr(x), _ptr(g), _ptr(dw), ctypes.byref(geom), self.dtype_code, cfg,
                     buf.wgrad_ws.data_ptr(), buf.wgrad_ws.numel(), st)

    def _plane_entry(self, name):
        """entry point `name` of the bf16 planes for this engine's plane format -> (entry point, it takes the format's scale)"""
        return F16_TWINS[name] if self.x3_f16 else (name, False)

    def _x3(self, name):
        """_plane_entry's entry point alone (tests launch plane helpers themselves)"""
        return self._plane_entry(name)[0]

    def _launch_plane(self, tag, name, args, scale, *tail):
        """args, [the fp16 twin's scale], tail: where every scaled twin takes it"""
        name, scaled = self._plane_entry(name)
        self._launch(tag, name, *args, *((scale,) if scaled else ()), *tail)

    def _split_planes(self, tag, src, dst, mask, batch, t_out, channels, src_batch_stride, dst_row0, dst_batch_stride, mode, st):
        """fp32 rows (the staging buffer) into planes, through the activation / its derivative of `mode` (_lib.SPLIT_*)"""
        self._launch_plane(tag, "sl_split3", (_ptr(src), _ptr(dst), _ptr(mask), batch, t_out, channels, src_batch_stride,
                                              dst_row0, dst_batch_stride, mode), None, st)

    def _pack_input_x3(self, src, buf, t_in, f, st):
        p0 = self.plans[0]
        self._launch_plane("pack_input", "sl_split3_pack_input", (src.data_ptr(), buf.x0.data_ptr(), buf.batch, t_in, f,
                           p0.cin_pad, p0.pad_left, buf.rows0 * p0.cin_pad * self.planes), None, st)

    def _dropout_x3(self, tag, src, dst, y, channels, mode, seed, st):
        """sl_split3_dropout (mode: _lib.DROP_*) over a whole plane tensor (halo rows and padding included: zeros stay zeros)"""
        self._launch_plane(tag, "sl_split3_dropout", (src.data_ptr(), dst.data_ptr(), _ptr(y),
                           src.numel() // (self.planes * channels), channels, mode, self.dropout_rate, seed), None, st)

    def _pack_weights_x3(self, tag, w_master, w_fwd, w_dgrad, k, cin, cout, st):
        """both operand copies [w_hi | w_hi | w_lo] of one layer from its fp32 master (f16x3: of w_scale * w)"""
        self._launch_plane(tag, "sl_split3_pack_weights", (w_master.data_ptr(), w_fwd.data_ptr(), _ptr(w_dgrad), k, cin, cout),
                           self.w_scale, st)

    def _combine_x3(self, tag, ra, rb, dw, taps, c_in, c_out, frames, fstride, ra_cin, rb_cin, rb_fstride, scale, st):
        """dW from the partial sums RA, RB; scale divides out what the operands were stored multiplied by (f16x3)"""
        self._launch_plane(tag, "sl_split3_wgrad_combine", (ra.data_ptr(), rb.data_ptr(), dw.data_ptr(), taps, c_in, c_out,
                           frames, fstride, ra_cin, rb_cin, rb_fstride), scale, st)

    def _bias_grad_x3(self, tag, g, db, batch, t_out, channels, g_row0, g_batch_stride, st):
        """db from the planes of g (f16x3: stored as g_scale * g); the workspace is allocated on first use"""
        if self._x3_bias_ws is None:
            self._x3_bias_ws = torch.empty((self.lib.raw("sl_split3_bias_grad_workspace_bytes")(
                max(q.cout_pad for q in self.plans)),), dtype=torch.uint8, device=self.device)
        self._launch_plane(tag, "sl_split3_bias_grad", (g.data_ptr(), db.data_ptr(), batch, t_out, channels, g_row0,
                           g_batch_stride), 1.0 / self.g_scale, self._x3_bias_ws.data_ptr(), self._x3_bias_ws.numel(), st)

    # ------------------------------------------------------------------ layer steps
    def _wgrad_bias_x3(self, buf, name, x, x_b, g, dw, db, geom_a, geom_b, taps, c_in, c_out, frames, fstride, rb_fstride,
                       dw_scale, t_out, g_row0, g_batch_stride, cfg, st):
        """Weight and bias gradient of one layer on the planes: RA = x planes [hi | lo] against g_hi, RB = x_b (the hi plane
        of x, or its window) against g_lo, the combine into dw (frames, fstride, rb_fstride: the pair view of a striding layer),
        then db from g at rows g_row0 .. + t_out (db None: the bias gradient comes out of dW's ones row)."""
        ra = buf.wgrad_r
        rb = ra[(taps // frames) * geom_a.cin * c_out:]
        self._wgrad(buf, "wgrad:" + name, x, g, ra, geom_a, cfg, st)
        self._wgrad(buf, "wgrad_lo:" + name, x_b, g.data_ptr() + c_out * 2, rb, geom_b, cfg, st)  # plane P1 of every row
        self._combine_x3("combine:" + name, ra, rb, dw, taps, c_in, c_out, frames, fstride, geom_a.cin, geom_b.cin, rb_fstride,
                         dw_scale, st)
        if db is not None:
            self._bias_grad_x3("bgrad:" + name, g, db, buf.batch, t_out, c_out, g_row0, g_batch_stride, st)

    def _dgrad_through(self, buf, name, g, w, y_prev, out, geom, activation, dropped, seed, cfg, st):
        """Single plane: the input gradient of a layer into `out`, through the activation that produced its input y_prev and
        the Dropout (dropped) between the two.  ReLU: the epilogue's mask (stored activation > 0) is the keep mask too, what is
        left of d dropout / dx is 1 / (1 - rate).  A stored zero is ambiguous behind an ELU (dropped, or elu(z) == 0): plain
        input gradient, then both factors of the chain rule with the keep decisions recomputed from the step's seed."""
        elu_dropped = activation == "elu" and dropped
        self._nt(buf, "dgrad:" + name, g, w, None, None if elu_dropped else y_prev, out, geom,
                 _lib.EPI_NONE if elu_dropped else mask_epilogue(activation), _lib.NT_OUT_ELEM, cfg, st)
        if elu_dropped:
            self._launch("dropout_elu_bwd:" + name, "sl_elu_dropout_backward", out.data_ptr(), y_prev.data_ptr(), out.numel(),
                         self.dtype_code, self.dropout_rate, seed, st)
        elif dropped:
            self._launch("dropout_scale:" + name, "sl_scale", out.data_ptr(), out.numel(), self.dtype_code,
                         1.0 / (1.0 - self.dropout_rate), st)

    def _dgrad_through_x3(self, buf, name, g, w, y_prev, out, geom, plane_geom, activation, dropped, seed, cfg, rows, channels,
                          src_batch_stride, dst_row0, dst_batch_stride, st):
        """_dgrad_through on the planes.  plane_geom (ReLU only): mask and split into planes in the NT kernel's epilogue;
        None: fp32 into the staging buffer (geom), then sl_split3 of `rows` rows per utterance through the mask into `out`."""
        elu_dropped = activation == "elu" and dropped
        if plane_geom is not None:
            self._nt(buf, "dgrad:" + name, g, w, None, y_prev, out, plane_geom, _lib.EPI_RELU_MASK, _lib.NT_OUT_PLANES, cfg, st)
        else:
            self._nt(buf, "dgrad:" + name, g, w, None, None, buf.stage32, geom, _lib.EPI_NONE, _lib.NT_OUT_F32, cfg, st)
            mode = _lib.SPLIT_COPY if elu_dropped else (_lib.SPLIT_ELU_MASK if activation == "elu" else _lib.SPLIT_RELU_MASK)
            self._split_planes("split:dgrad:" + name, buf.stage32, out, None if elu_dropped else y_prev, buf.batch, rows, channels,
                               src_batch_stride, dst_row0, dst_batch_stride, mode, st)
        if elu_dropped:
            self._dropout_x3("dropout_elu_bwd:" + name, out, out, y_prev, channels, _lib.DROP_ELU_BACKWARD, seed, st)
        elif dropped:
            self._dropout_x3("dropout_scale:" + name, out, out, None, channels, _lib.DROP_SCALE, 0, st)

    # ------------------------------------------------------------------ the frame of the forward and backward loops
    def _forward_prologue(self, buf, rate, st):
        """the dropout step counter and seed, the front layer, the Dropout on the packed input -> (input of layer 0, seed0)"""
        seed0 = 0
        if rate:
            self._dropout_steps += 1
            # (kept on the buffer set: backward behind an ELU recomputes the keep decisions)
            seed0 = buf.dropout_seed0 = (self.dropout_seed * 1000003 + self._dropout_steps) * 64
        if self.front_plan is not None:
            self._front_forward(buf, rate, seed0, st)
        if not rate:
            return buf.x0, seed0
        if buf.x0_dropped is None:
            buf.x0_dropped = torch.zeros_like(buf.x0)
        if self.planes > 1:
            self._dropout_x3("dropout:input", buf.x0, buf.x0_dropped, None, self.plans[0].cin_pad, _lib.DROP_FORWARD, seed0, st)
        else:
            self._launch("dropout:input", "sl_dropout", buf.x0.data_ptr(), buf.x0_dropped.data_ptr(), buf.x0.numel(),
                         self.dtype_code, rate, seed0, st)
        return buf.x0_dropped, seed0

    def _launch_softmax(self, buf, st):
        cp = self.plans[-1].cout_pad
        self._launch("softmax", "sl_softmax_logq", buf.logits.data_ptr(), buf.probs.data_ptr(), buf.logq.data_ptr(), buf.batch,
                     buf.t_out, self.grapheme_set_size, cp, buf.tt_pad * cp, self.ctc_epsilon, st)

    def _close_bucket(self, on_bucket_ready, b, layers, ones_in, ones_db, main, join_side=None):
        """every launch that writes bucket b = `layers` is enqueued on MAIN but the bias rows out of its weight gradients"""
        rows = [j for j in layers if j in ones_in]
        if rows:
            self._bias_grads_from_wgrad(rows, bool(ones_db), main)
        if join_side is not None:
            join_side()
        self._bucket_ready(on_bucket_ready, b)
        if self.comm_cus and b == 0:  # from here on communication kernels may own CUs: the choosers plan for the rest
            self._eager_op(self._set_cu_hint, 256 - self.comm_cus)

    def _backward_tail(self, buf, on_bucket_ready, ones_in, ones_db, main, join_side=None):
        """behind the stack's loop: the bias rows nobody closed a bucket for, the front layer and its bucket, the CU hint"""
        if on_bucket_ready is None:
            if ones_in:
                self._bias_grads_from_wgrad(ones_in, bool(ones_db), main)
            if join_side is not None:
                join_side()
        if self.front_plan is not None and self.frozen_layer_count == 0 and not self.front_frozen:
            self._front_backward(buf, main.cuda_stream)
            if on_bucket_ready is not None:  # the front layer's parameters: the last bucket of bucket_plan()
                self._bucket_ready(on_bucket_ready, len(self.bucket_plan()) - 1)
        if on_bucket_ready is not None and self.comm_cus:
            self._eager_op(self._set_cu_hint, 0)
