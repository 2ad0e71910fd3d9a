"""The bf16x3 path of the engine (Engine(dtype="bf16x3")): every fp32 value as hi + lo bf16 planes, a product as three bf16 MFMA
terms through the unchanged NT / TN kernels (csrc/split3.hip; DESIGN.md section 3.1, HISTORY.md section 3.6).  Methods of Engine."""
import torch

from . import _lib
from .plan import HALO


class X3Mixin:
    def _repack_weights_x3(self):
        """bf16x3 operand copies: rows [w_hi | w_hi | w_lo] in both operand layouts, w_hi = bf16(w), w_lo = bf16(w - w_hi),
        one launch per layer (sl_split3_pack_weights; the five-launch sequence it replaces -- split, two packs, two
        assembles -- was 55 launches and 0.45 ms of a 7.1 ms optimisation step)."""
        st = self._stream()
        for p in self.all_plans:  # (the raw-wave front layer included; a striding layer with a dgrad operand: its pair view)
            wv, _ = self.layer_param_views(self.params, p)
            wd = self.w_dgrad[p.index]
            if p.index == 0 and p is not self.front_plan:
                wd = None  # (only there under a front layer, and then in the pair view: _pack_pair_dgrad_x3 below)
            k, cin = self._pack_dims(p)
            self._pack_weights_x3("pack3:" + p.spec.name, wv, self.w_fwd[p.index], wd, k, cin, p.cout_pad, st)
        if self.w_dgrad[0] is not None:
            self._pack_pair_dgrad_x3(st)
        self._packed_dirty = False

    def _pack_pair_dgrad_x3(self, st):
        """the input-gradient operand of the striding layer under a raw-wave front layer: the PAIR VIEW of its taps (24 flipped
        pair taps x 2 cin_pad pair channels, rows [w_hi | w_hi | w_lo] over the output channels) -- sl_split3_pack_weights on
        the pair view of the masters; the forward operand it writes beside it goes to a scratch buffer (the layer's real
        forward operand is packed with its own 48 taps: a frame's planes are contiguous in a row of the input buffer)"""
        p0 = self.plans[0]
        if getattr(self, "_w_fwd0_pair_scratch", None) is None:
            self._w_fwd0_pair_scratch = torch.empty_like(self.w_fwd[0])
        wv, _ = self.layer_param_views(self.params, p0)
        self._pack_weights_x3("pack3_pair:" + p0.spec.name, wv, self._w_fwd0_pair_scratch, self.w_dgrad[0], p0.taps_view,
                              p0.cin_view, p0.cout_pad, st)

    def _plane_geom(self, buf, kind, i, channels):
        """the NT geometry of layer i (kind 'fwd' / 'dgrad') with its OUTPUT side describing a bf16x3 plane tensor of
        `channels` padded channels (rows of 3 x channels behind HALO halo rows) instead of the fp32 staging buffer"""
        g = buf.plane_geoms.get((kind, i))
        if g is None:
            src = (buf.fwd_geom if kind == "fwd" else buf.dgrad_geom)[i]
            g = src.copy()
            g.y_row0, g.y_row_stride, g.y_batch_stride = HALO, self.planes * channels, buf.rows * channels * self.planes
            buf.plane_geoms[(kind, i)] = g
        return g

    def _forward_x3(self, buf, st, rate=None):
        """bf16x3: every layer = the unchanged NT kernel over the three planes.  ReLU layers: bias, ReLU and the split into
        planes in the kernel's own epilogue (out_f32 = 2); ELU layers: fp32 into the staging buffer + sl_split3.  The last
        layer's fp32 logits go to the softmax as on the other paths.  Dropout (training, net.py:301-303): sl_split3_dropout
        on the packed input (into a second buffer) and in place on every activation that feeds a layer with a Dropout in
        front of it -- the same (seed, element) keep decisions as sl_dropout draws on the single-plane paths."""
        n = len(self.plans)
        x, seed0 = self._forward_prologue(buf, rate, st)
        for p in self.plans:
            last = p.index == n - 1
            _, bias = self.layer_param_views(self.params, p)
            cfg = self.nt_cfg.get(("fwd", p.spec.name), 0)
            name, w, geom = p.spec.name, self.w_fwd[p.index], buf.fwd_geom[p.index]
            if last:
                self._nt(buf, "fwd:" + name, x, w, bias, None, buf.logits, geom, _lib.EPI_BIAS, _lib.NT_OUT_F32, cfg, st)
                break
            y = buf.y[p.index]
            if p.spec.activation == "relu" and self.x3_fused_epilogue:
                self._nt(buf, "fwd:" + name, x, w, bias, None, y, self._plane_geom(buf, "fwd", p.index, p.cout_pad),
                         _lib.EPI_BIAS_RELU, _lib.NT_OUT_PLANES, cfg, st)
            else:
                self._nt(buf, "fwd:" + name, x, w, bias, None, buf.stage32, geom, _lib.EPI_BIAS, _lib.NT_OUT_F32, cfg, st)
                self._split_planes("split:" + name, buf.stage32, y, None, buf.batch, buf.t_out, p.cout_pad, buf.tt_pad * p.cout_pad,
                                   HALO, buf.rows * p.cout_pad * self.planes,
                                   _lib.SPLIT_ELU if p.spec.activation == "elu" else _lib.SPLIT_RELU, st)
            if rate and (p.index + 1) in self._dropout_layers():
                self._dropout_x3("dropout:" + name, y, y, None, p.cout_pad, _lib.DROP_FORWARD, seed0 + p.index + 1, st)
            x = y
        self._launch_softmax(buf, st)
        return buf.probs

    def _backward_x3(self, buf, st, on_bucket_ready=None):
        """bf16x3 backward: per layer the weight gradient of the [hi | lo] prefixes + sl_split3_wgrad_combine, the input
        gradient through the unchanged NT kernel (fp32 staging) + sl_split3 with the activation mask.  Bias gradients:
        row cin_pad - 1 of dW where the input carries the ones channel (hi = 1, lo = 0), sl_split3_bias_grad elsewhere (and
        everywhere when dropout touched the ones).  Everything runs on ONE stream, so a gradient bucket (bucket_plan) is
        complete the moment the launches of its lowest layer are enqueued: on_bucket_ready(b) is called there, exactly as
        _backward_eager does for the single-plane paths."""
        first = self.frozen_layer_count
        pl = self.planes
        ones_in = self._ones_input_layers(first)
        ones_db = set() if buf.dropped else set(ones_in)  # rows that hold a bias gradient (else: only to be zeroed)
        main = torch.cuda.current_stream(self.device)
        plan = self.bucket_plan() if on_bucket_ready is not None else []
        bucket_at = {layers[0]: (b, layers) for b, (layers, _) in enumerate(plan)}
        # the runs of identical layers (inner_conv_1..7): their 2 x 7 partial weight gradients (x planes against g_hi, against
        # g_lo) in ONE balanced launch (sl_conv1d_wgrad_multi, a job per partial) at the lowest layer of the run -- they
        # were 14 launches of 31 us + their reductions, 0.6 ms of the 6.8 ms step
        multi = {}
        for launch_layers in self._x3_multi_runs(first):
            for i in launch_layers:
                multi[i] = launch_layers
        for p in reversed(self.plans[first:]):
            i = p.index
            name = p.spec.name
            x = (buf.x0_dropped if buf.dropped else buf.x0) if i == 0 else buf.y[i - 1]
            dw, db = self.layer_param_views(self.grads, p)
            if i in ones_db:
                db = None  # (out of row cin_pad - 1 of dW)
            g_stride = buf.rows * p.cout_pad * pl
            if i in multi:
                if i == multi[i][0]:  # every gradient tensor of the run is complete here
                    self._launch_wgrad_multi_x3(buf, multi[i], st)
                if db is not None:
                    self._bias_grad_x3("bgrad:" + name, buf.g[i], db, buf.batch, buf.t_out, p.cout_pad, HALO, g_stride, st)
            else:
                # the striding layer's pair view: two frames' planes per row; RB's x operand may be the [hi0 | hi1] window of
                # the pair row (buf.x3_window)
                frames = 2 if p.spec.stride == 2 else 1
                fstride = pl * p.cin_pad if frames == 2 else 0
                window = frames == 2 and buf.x3_window
                x_b = x.data_ptr() + (2 * p.cin_pad * 2 if (i == 0 and window) else 0)
                self._wgrad_bias_x3(buf, name, x, x_b, buf.g[i], dw, db, buf.wgrad_geom[i], buf.wgrad_geom_b[i],
                                    p.spec.kernel_size, p.cin_pad, p.cout_pad, frames, fstride, p.cin_pad if window else fstride,
                                    1.0 / self.g_scale, buf.t_out, HALO, g_stride, self.nt_cfg.get(("wgrad", name), 0), st)
            if i in bucket_at:
                self._close_bucket(on_bucket_ready, *bucket_at[i], ones_in, ones_db, main)
            if i > first:
                fused = self.specs[i - 1].activation == "relu" and self.x3_fused_epilogue
                self._dgrad_through_x3(buf, name, buf.g[i], self.w_dgrad[i], buf.y[i - 1], buf.g[i - 1], buf.dgrad_geom[i],
                                       self._plane_geom(buf, "dgrad", i, p.cin_pad) if fused else None,
                                       self.specs[i - 1].activation, buf.dropped and i in self._dropout_layers(),
                                       buf.dropout_seed0 + i, self.nt_cfg.get(("dgrad", name), 0), buf.t_out, p.cin_pad,
                                       buf.tt_pad * p.cin_pad, HALO, buf.rows * p.cin_pad * pl, st)
        self._backward_tail(buf, on_bucket_ready, ones_in, ones_db, main)

    def _launch_wgrad_multi_x3(self, buf, layers, st):
        """bf16x3: the partial weight gradients RA (x planes [hi | lo] against g_hi) and RB (x plane hi against g_lo) of
        every layer of a run as jobs of one sl_conv1d_wgrad_multi launch, then sl_split3_wgrad_combine per layer"""
        key = ("x3", buf.dropped) + tuple(layers)
        entry = buf.multi_tables.get(key)
        if entry is None:
            sizes = [(self.plans[i].taps_view * buf.wgrad_geom[i].cin * self.plans[i].cout_pad,
                      self.plans[i].taps_view * buf.wgrad_geom_b[i].cin * self.plans[i].cout_pad) for i in layers]
            scratch = torch.empty((sum(a + b for a, b in sizes),), dtype=torch.float32, device=self.device)
            table = (_lib.WgradJob * (2 * len(layers)))()
            parts, off = [], 0
            for n, (i, (na, nb)) in enumerate(zip(layers, sizes)):
                ra, rb = scratch[off:off + na], scratch[off + na:off + na + nb]
                off += na + nb
                parts.append((ra, rb))
                x = (buf.x0_dropped if buf.dropped else buf.x0) if i == 0 else buf.y[i - 1]
                for job, (g_ptr, out, geom) in zip((table[2 * n], table[2 * n + 1]),
                                                   ((buf.g[i].data_ptr(), ra, buf.wgrad_geom[i]),
                                                    (buf.g[i].data_ptr() + self.plans[i].cout_pad * 2, rb,
                                                     buf.wgrad_geom_b[i]))):
                    job.x, job.g, job.dw = x.data_ptr(), g_ptr, out.data_ptr()
                    job.geom.copy_from(geom)
            need = self._wgrad_multi_workspace_need(table, len(table))
            ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
            entry = buf.multi_tables[key] = (table, parts, scratch, ws)
        table, parts, _, ws = entry
        self._launch("wgrad:{}..{}".format(self.specs[layers[0]].name, self.specs[layers[-1]].name),
                     "sl_conv1d_wgrad_multi", table, len(table), self.dtype_code, ws.data_ptr(), ws.numel(), st)
        for i, (ra, rb) in zip(layers, parts):  # (stride-1 layers, _x3_multi_runs: one frame per row, no window)
            p = self.plans[i]
            dw, _ = self.layer_param_views(self.grads, p)
            self._combine_x3("combine:" + p.spec.name, ra, rb, dw, p.spec.kernel_size, p.cin_pad, p.cout_pad, 1, 0,
                             buf.wgrad_geom[i].cin, buf.wgrad_geom_b[i].cin, 0, 1.0 / self.g_scale, st)
