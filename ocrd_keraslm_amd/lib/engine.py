"""HipLM: the MI355X engine behind `Rater.model`.

Plays the role the compiled Keras model plays in the reference
(ocrd_keraslm/lib/rating.py:56, 171-178): it owns the weights, the optimizer
moments, the implicit LSTM state of stateful streams and the state pool of
incremental hypotheses -- all as torch tensors in HBM -- and runs every
contraction through the hand-written gfx950 kernels behind the C ABI
(include/keraslm_hip.h).  torch is used for device memory, streams and (in
`distributed.py`) the RCCL all-reduce only.  There is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import time

import numpy as np

from . import hipabi, ratebulk

CTX_VOCAB = 200   # rating.py:111
CTX_DIM = 10
DROPOUT_RATE = 0.1  # rating.py:152


FAST_WIDTHS = (64, 128, 256, 512, 1024)   # hidden sizes the persistent scans are instantiated for


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# what the builders of hypothesis rows say of their tensors (the call's name, its own tensors)
_HYPOTHESIS_TENSORS = ("%s: corpus int32 [n], offsets int64 [n_texts + 1], text_ctx int32 [n_texts, n_ctx], %s, contiguous, "
                       "on the device")


def physical_width(width):
    """The width the kernels run at: the next one the persistent scans serve (else the next multiple of 32).
    The extra hidden units are zero-padding -- all their weights and biases are zero, so their cell and
    output stay exactly zero, nothing flows out of them, and their gradients are exactly zero (Adam leaves
    them alone): a model of ANY width (the reference takes 1..9128, scripts/run.py:34) runs bit-identically to
    its padded twin, on the fast kernels."""
    for w in FAST_WIDTHS:
        if width <= w:
            return w
    return (width + 31) // 32 * 32


def _solve_lower(low, rhs):
    """low^-1 rhs for a lower triangular matrix"""
    from scipy.linalg import solve_triangular
    return solve_triangular(low, rhs, lower=True, check_finite=False)


class HipLM:
    def __init__(self, depth, width, voc_size, n_ctx=1, device="cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise hipabi.KlError("no GPU visible: the Rater hot path runs on MI355X only (no CPU fallback)")
        self.torch = torch
        self.lib = hipabi.load()
        self.device = torch.device(device)
        self.depth, self.width, self.voc_size, self.n_ctx = int(depth), int(width), int(voc_size), int(n_ctx)
        if self.width < 1:
            raise hipabi.KlError("width must be positive (got %d)" % self.width)
        self.pwidth = physical_width(self.width)       # what the kernels see (zero-padded hidden units)
        self.padded = self.pwidth != self.width
        self.cfg = hipabi.KlConfig(self.depth, self.pwidth, self.voc_size, self.n_ctx, CTX_VOCAB, CTX_DIM)
        self.handle = self.lib.kl_create(C.byref(self.cfg))
        if not self.handle:
            raise hipabi.KlError("kl_create rejected configuration depth=%d width=%d voc=%d"
                                 % (self.depth, self.width, self.voc_size))
        self.n_params = self.lib.kl_param_count(C.byref(self.cfg))
        self.layout = self._read_layout()
        # all launches go to one side stream: whole windows are replayed as hipGraphs,
        # and the legacy default stream cannot be captured
        self.stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.device(self.device):
            self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
            nbytes = self.lib.kl_derived_bytes(self.handle)
            self.derived = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            hipabi.check(self.lib.kl_bind(self.handle, _ptr(self.params), _ptr(self.derived), nbytes), "kl_bind")
        self.precision = 0
        self.grads = None
        self.adam_m = None
        self.adam_v = None
        self.adam_t = 0
        self.loss_acc = torch.zeros(4, dtype=torch.float32, device=self.device)
        for slot in self._WS_SLOTS.values():      # (the workspace buffers and what they were sized for: _workspace)
            setattr(self, slot, None)
            setattr(self, slot + "_key", None)
        self.rate_bits = None       # [B] f64: bits per stream accumulated by rate_window
        self._rate_status = None
        self._rate_select_ws = None
        self._word_bounds_ws = None
        self._segment_select_ws = None
        self._lexicon_ws = None
        self._lexicon_channel_ws = None
        self._lexicon_splits_ws = None
        self._lexicon_chains_ws = None
        self._align_ws = None
        self._confusion_ws = None
        self._witness_ws = None
        self.states = None       # [B][2L][W] implicit state of the stateful streams
        self.pool = None            # [slots][2L][W] explicit states of hypotheses
        self.max_streams_per_launch = 0      # 0: what the kernels address (train_window splits larger batches into groups)
        self._part_grads = None
        self._part_loss = None
        self._pad_states = {}
        self._fan_states = {}                # rows -> the state buffer `fan_states` fills for that many streams
        self.pad_streams = True              # pad a group of streams up to the next fast count (HipLM._padded_streams)
        self.plan_override = None            # width 512: a stream plan to use instead of _plan_512's (tests)
        self.group_hook = None               # tests: called per stream group of a grouped window (see window_view)
        self._step_ws = None
        self._step_host_ws = None
        self._walk_ws = None
        self._beam_ws = None
        self._sample_ws = None
        self._wstage = None
        self._hio = None
        self._step_ws_bytes = {}
        self.last_only = False
        self._last_window = None    # (streams run, T, first real stream, real streams, groups) of the last train_window
        self._last_forward = None   # (streams, T, workspace) of the last inference-layout window (forward_window, rate_window[_alts])
        self._rng = np.random.default_rng(0)

    def __del__(self):
        try:
            if getattr(self, "_hio", None) is not None:
                self._host_io_free()
            if getattr(self, "_wstage", None) is not None:
                self.torch.cuda.synchronize(self.device)
                self.lib.kl_host_free(self._wstage[0])
                self._wstage = None
            if getattr(self, "handle", None):
                self.lib.kl_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _read_layout(self):
        out = []
        i = 0
        name = C.create_string_buffer(32)
        off, rows, cols = C.c_size_t(), C.c_size_t(), C.c_size_t()
        while self.lib.kl_param_layout(C.byref(self.cfg), i, name, 32, C.byref(off), C.byref(rows), C.byref(cols)) == 0:
            out.append((name.value.decode(), off.value, rows.value, cols.value))
            i += 1
        return out

    def _stream(self):
        return C.c_void_p(self.stream.cuda_stream)

    @contextlib.contextmanager
    def _launch(self):
        """Run the enclosed launches on the engine stream, ordered after what the
        caller's current stream has enqueued and before what it enqueues next."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                yield
        finally:
            cur.wait_stream(self.stream)      # (also when the body raised: the streams stay joined)

    # `layout`, `params`, `grads`, `states`, `pool` are PHYSICAL (padded width); the accessors below speak the
    # model's own shapes.  For the widths in FAST_WIDTHS (and multiples of 32 above 1024) both coincide.
    def _logical_shape(self, name):
        W = self.width
        if name == "E":
            return (self.voc_size, W)
        if name.startswith("Ctx"):
            return (CTX_VOCAB, CTX_DIM)
        if name.startswith("b"):
            return (4 * W,)
        if name == "K0":
            return (W + self.n_ctx * CTX_DIM, 4 * W)
        return (W, 4 * W)

    def _row_map(self, name, n_rows):
        """physical row of every logical row (K0: the context rows sit behind the padded embedding rows)"""
        r = np.arange(n_rows)
        if name == "K0":
            r = np.where(r < self.width, r, r + (self.pwidth - self.width))
        return r

    def _pad(self, name, a):
        """logical array -> physical array (zeros in the padding)"""
        a = np.asarray(a, dtype=np.float32).reshape(self._logical_shape(name))
        if not self.padded or name.startswith("Ctx"):
            return a
        W, Wp = self.width, self.pwidth
        if name == "E":
            out = np.zeros((a.shape[0], Wp), dtype=np.float32)
            out[:, :W] = a
            return out
        if name.startswith("b"):
            out = np.zeros(4 * Wp, dtype=np.float32)
            for g in range(4):
                out[g * Wp:g * Wp + W] = a[g * W:(g + 1) * W]
            return out
        rows = self._row_map(name, a.shape[0])
        out = np.zeros((a.shape[0] + (Wp - W), 4 * Wp), dtype=np.float32)
        for g in range(4):
            out[rows, g * Wp:g * Wp + W] = a[:, g * W:(g + 1) * W]
        return out

    def _unpad(self, name, a):
        """physical array -> logical array"""
        if not self.padded or name.startswith("Ctx"):
            return a
        W, Wp = self.width, self.pwidth
        if name == "E":
            return a[:, :W].copy()
        if name.startswith("b"):
            return np.concatenate([a[g * Wp:g * Wp + W] for g in range(4)])
        rows = self._row_map(name, self._logical_shape(name)[0])
        return np.concatenate([a[rows, g * Wp:g * Wp + W] for g in range(4)], axis=1)

    def _unflatten(self, flat):
        out = {}
        for name, off, rows, cols in self.layout:
            a = flat[off:off + rows * cols]
            a = a.reshape(cols).copy() if name.startswith("b") else a.reshape(rows, cols).copy()
            out[name] = self._unpad(name, a)
        return out

    def get_weights(self):
        """dict name -> float32 array in Keras shapes (E, Ctx0.., K0, U0, b0, ...)."""
        return self._unflatten(self.params.detach().cpu().numpy())

    def get_grads(self):
        """gradients of the last train_window, same names and shapes as get_weights()"""
        return self._unflatten(self.grads.detach().cpu().numpy())

    def set_weights(self, weights, precision=None):
        flat = np.empty(self.n_params, dtype=np.float32)
        for name, off, rows, cols in self.layout:
            a = np.asarray(weights[name], dtype=np.float32)
            if a.size != int(np.prod(self._logical_shape(name))):
                raise ValueError("weight %s has %d elements, expected shape %s" % (name, a.size, self._logical_shape(name)))
            flat[off:off + rows * cols] = self._pad(name, a).reshape(-1)
        with self._launch():
            self.params.copy_(self.torch.from_numpy(flat))
        self.prepare(precision or self.precision or hipabi.KL_PREC_SPLIT)

    def get_states(self):
        """implicit states of the stateful streams, numpy [B][2L][W]"""
        return self.states[:, :, :self.width].cpu().numpy()

    def set_states(self, values):
        values = np.asarray(values, dtype=np.float32)
        self.reset_states(values.shape[0])
        with self._launch():
            self.states[:, :, :self.width] = self.torch.from_numpy(np.ascontiguousarray(values)).to(self.device)

    def init_weights(self, seed=None, emb_std=0.001):
        """Keras initialisers of rating.py:104-114 + LSTM defaults (glorot_uniform kernel,
        orthogonal recurrent kernel, zero bias with unit forget gate)."""
        rng = np.random.default_rng(seed)
        W = self.width
        w = {}
        for name, _off, _rows, _cols in self.layout:
            shape = self._logical_shape(name)
            rows, cols = (1, shape[0]) if len(shape) == 1 else shape
            if name == "E" or name.startswith("Ctx"):
                w[name] = (rng.standard_normal((rows, cols)) * emb_std).astype(np.float32)
            elif name.startswith("K"):
                lim = math.sqrt(6.0 / (rows + cols))
                w[name] = rng.uniform(-lim, lim, (rows, cols)).astype(np.float32)
            elif name.startswith("U"):
                # Keras' Orthogonal: the Q of a QR factorisation of a [4W, W] Gaussian matrix, signs fixed so that R's diagonal
                # is positive.  That factorisation is unique, and for such a well-conditioned matrix (condition number 3) it is
                # had from a Cholesky factor of the Gram matrix -- matrix products instead of Householder steps (0.28 s each
                # at width 512).  Done twice, the second pass removes the rounding of the first.
                a = rng.standard_normal((cols, rows))
                qt = a.T
                for _ in range(2):
                    low = np.linalg.cholesky(qt @ qt.T)
                    qt = _solve_lower(low, qt)
                w[name] = qt.astype(np.float32)
            else:
                b = np.zeros(cols, dtype=np.float32)
                b[W:2 * W] = 1.0
                w[name] = b
        self.set_weights(w, self.precision or hipabi.KL_PREC_SPLIT)

    def prepare(self, precision):
        with self._launch():
            hipabi.check(self.lib.kl_prepare(self.handle, int(precision), self._stream()), "kl_prepare")
        self.precision = int(precision)

    # ------------------------------------------------------------------ windows
    # kl_<kind>_workspace_bytes -> the attribute that holds the kind's buffer (its key in <attribute>_key)
    _WS_SLOTS = {"window": "_ws", "rate": "_rate_ws", "rate_alts": "_rate_alts_ws", "rate_alts_bulk": "_rate_alts_bulk_ws"}

    def _workspace(self, B, T, *tail, kind="window"):
        """the kind's workspace for B streams of T characters, kept until another size is asked for.  tail: what else its size
        depends on -- (training,) for "window", () for "rate", (k,) for "rate_alts" and "rate_alts_bulk"."""
        slot = self._WS_SLOTS[kind]
        key = (B, T) + tail
        if getattr(self, slot + "_key") != key:
            n = getattr(self.lib, "kl_%s_workspace_bytes" % kind)(self.handle, B, T, *map(int, tail))
            setattr(self, slot, None)      # (the old buffer goes back to the allocator before the new one is taken)
            setattr(self, slot, self.torch.empty(n, dtype=self.torch.uint8, device=self.device))
            setattr(self, slot + "_key", key)
        return getattr(self, slot)

    def _pad_group(self, b0, b1, Bp, idx_d, ctx_d, tgt_d, fill):
        """streams [b0, b1) of a batch as a group of Bp >= b1 - b0: returns (idx, ctx, tgt, states) of the group, ctx and tgt None
        where the batch has none.  Bp beyond the real streams are dummy streams: idx 0, ctx 0, tgt `fill`, zero state -- the
        states then a buffer of their own (one per padded count: its address is part of the replayed launch sequence's key)
        that `_unpad_states` copies back."""
        torch = self.torch
        n = b1 - b0
        x, st = idx_d[b0:b1], self.states[b0:b1]
        c = ctx_d[b0:b1] if ctx_d is not None else None
        y = tgt_d[b0:b1] if tgt_d is not None else None
        if Bp != n:
            x = torch.nn.functional.pad(x, (0, 0, 0, Bp - n))
            if y is not None:
                y = torch.nn.functional.pad(y, (0, 0, 0, Bp - n), value=fill)
            if c is not None:
                c = torch.nn.functional.pad(c, (0, 0) * (c.dim() - 1) + (0, Bp - n))
            st = self._pad_states.get(Bp)
            if st is None:
                st = self._pad_states[Bp] = torch.zeros((Bp,) + tuple(self.states.shape[1:]), dtype=torch.float32,
                                                        device=self.device)
            st[:n] = self.states[b0:b1]
            st[n:] = 0
        return x, c, y, st

    def _unpad_states(self, b0, b1, st):
        if st.shape[0] != b1 - b0:
            self.states[b0:b1] = st[:b1 - b0]

    def set_window_mode(self, last_only):
        """False (default): the stateful graph -- a target at every position, means over B*T positions.
        True: the stateless graph (rating.py:126-129) -- one target per window at its last position,
        means over the B windows."""
        hipabi.check(self.lib.kl_set_window_mode(self.handle, 1 if last_only else 0), "kl_set_window_mode")
        self.last_only = bool(last_only)

    def reset_states(self, B=None, rows=None):
        """Keras reset_states (rating.py:475, 555; callbacks.py:58, 69)."""
        if self.states is None or (B is not None and self.states.shape[0] != B):
            self.states = self.torch.zeros((B or 1, 2 * self.depth, self.pwidth), dtype=self.torch.float32,
                                           device=self.device)
        elif rows is None:
            self.states.zero_()
        else:
            self.states[self.torch.as_tensor(rows, device=self.device, dtype=self.torch.long)] = 0

    def _dev_i32(self, a):
        if isinstance(a, self.torch.Tensor):
            return a.to(device=self.device, dtype=self.torch.int32).contiguous()
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def forward_window(self, idx, ctx, tgt=None, want_probs=True):
        """idx [B,T], ctx [B,T,n_ctx], tgt [B,T] (-1 = padded) or None.
        Returns probs [B,T,V] (numpy) or None; with tgt also accumulates loss_acc."""
        torch = self.torch
        if self.precision == 0:
            raise hipabi.KlError("weights not prepared")
        with self._launch():
            idx_d = self._dev_i32(idx)
            B, T = idx_d.shape
            ctx_d = self._dev_i32(ctx) if self.n_ctx else None
            tgt_d = self._dev_i32(tgt) if tgt is not None else None
            if self.states is None or self.states.shape[0] != B:
                self.reset_states(B)
            # (bf16 precision = validation windows: a training-size workspace lets the library take the training
            # forward, i.e. the persistent scans; it is the buffer train_window uses anyway)
            training_ws = self.precision == hipabi.KL_PREC_BF16
            probs = torch.empty((B, T, self.voc_size), dtype=torch.float32, device=self.device) if want_probs else None
            parts = self._stream_groups(B, T) if training_ws else self._rating_groups(B)
            # (validation windows -- bf16, a loss and no probabilities wanted -- are padded like training batches)
            padded = [self._padded_streams(b1 - b0, T) if (training_ws and not want_probs and tgt_d is not None) else b1 - b0
                      for b0, b1 in parts]
            if len(parts) == 1 and padded[0] == B:
                ws = self._workspace(B, T, training_ws)
                hipabi.check(self.lib.kl_forward_window(self.handle, B, T, _ptr(idx_d), _ptr(ctx_d), _ptr(tgt_d),
                                                        _ptr(self.states), _ptr(probs), _ptr(self.loss_acc), _ptr(ws),
                                                        ws.numel(), self._stream()), "kl_forward_window")
                if not training_ws:
                    self._last_forward = (B, T, ws)
            else:
                # (more streams than one launch sequence addresses: groups of streams one after the other, as in train_window;
                # the means over the batch are the size-weighted sums of the groups' means)
                if self._part_loss is None:
                    self._part_loss = torch.zeros_like(self.loss_acc)
                ws = self._workspace(max(padded), T, training_ws)
                for i, ((b0, b1), Bp) in enumerate(zip(parts, padded)):
                    n = b1 - b0
                    self._part_loss.zero_()
                    # (-2, not the -1 of a padded tail: a dummy stream is no hit for the accuracy either)
                    x, c, y, st = self._pad_group(b0, b1, Bp, idx_d, ctx_d, tgt_d, -2)
                    if Bp != n:
                        hipabi.check(self.lib.kl_set_loss_rows(self.handle, n), "kl_set_loss_rows")
                    try:
                        hipabi.check(self.lib.kl_forward_window(self.handle, Bp, T, _ptr(x), _ptr(c), _ptr(y), _ptr(st),
                                                                _ptr(probs[b0:b1] if probs is not None else None),
                                                                _ptr(self._part_loss), _ptr(ws), ws.numel(), self._stream()),
                                     "kl_forward_window")
                    finally:
                        if Bp != n:
                            hipabi.check(self.lib.kl_set_loss_rows(self.handle, 0), "kl_set_loss_rows")
                    if not training_ws:
                        self._last_forward = (Bp, T, ws)
                    self._unpad_states(b0, b1, st)
                    if self.group_hook is not None:
                        self.group_hook(i, b0, b1, Bp)
                    self.loss_acc[:2] += (n / B) * self._part_loss[:2]
                    self.loss_acc[3] = torch.maximum(self.loss_acc[3], self._part_loss[3])
            if want_probs and float(self.loss_acc[3].item()) != 0.0:
                # (the caller reads the probabilities next, so this sync is not an extra one)
                self.loss_acc[3] = 0.0        # one timed-out window must not fail every later call
                raise hipabi.KlError("persistent scan hand-off timed out (kl_forward_window)")
        return probs

    # ------------------------------------------------------------------ rating windows: one call, four deliveries
    def _rate_call(self, idx, ctx, tgt, k, bulk, want_probs=True):
        """What the four rate_window methods do.  k None: the target's probability only (tprob, or None without want_probs);
        else also the k most probable characters and the target's rank (tprob, alt_id, alt_p, rank).  bulk: on the bf16
        training forward, streams grouped and padded as `forward_window` does for validation windows, with the training
        window's workspace when k is None; else on the inference layout in `_rating_groups`, unpadded."""
        torch = self.torch
        if self.precision == 0:
            raise hipabi.KlError("weights not prepared")
        alts = k is not None
        if alts:
            k = int(k)
            if not 1 <= k <= hipabi.KL_RATE_ALTS_MAX:
                raise ValueError("k must be in 1..%d (got %d)" % (hipabi.KL_RATE_ALTS_MAX, k))
        if bulk and self.precision != hipabi.KL_PREC_BF16:
            self.prepare(hipabi.KL_PREC_BF16)
        name = "kl_rate_window" + ("_alts" if alts else "") + ("_bulk" if bulk else "")
        fn = getattr(self.lib, name)
        with self._launch():
            idx_d = self._dev_i32(idx)
            B, T = idx_d.shape
            ctx_d = self._dev_i32(ctx) if self.n_ctx else None
            tgt_d = self._dev_i32(tgt)
            if self.states is None or self.states.shape[0] != B:
                self.reset_states(B)
            if self.rate_bits is None or self.rate_bits.shape[0] != B:
                self.rate_bits = torch.zeros(B, dtype=torch.float64, device=self.device)
            if self._rate_status is None:
                self._rate_status = torch.zeros(4, dtype=torch.float32, device=self.device)
            # (streams are independent: more than one launch sequence takes run as groups, the batch-major outputs sliced by stream)
            parts = self._stream_groups(B, T) if bulk else self._rating_groups(B)
            padded = [self._padded_streams(b1 - b0, T) if bulk else b1 - b0 for b0, b1 in parts]
            if alts:
                ws = self._workspace(max(padded), T, k, kind="rate_alts_bulk" if bulk else "rate_alts")
                outs = [torch.empty((B, T) + tail, dtype=dtype, device=self.device) for tail, dtype in
                        (((), torch.float32), ((k,), torch.int32), ((k,), torch.float32), ((), torch.int32))]
            else:
                ws = self._workspace(max(padded), T, True) if bulk else self._workspace(max(padded), T, kind="rate")
                outs = [torch.empty((B, T), dtype=torch.float32, device=self.device)] if want_probs else []
            for (b0, b1), Bp in zip(parts, padded):
                n = b1 - b0
                x, c, y, st = self._pad_group(b0, b1, Bp, idx_d, ctx_d, tgt_d, -1)
                out, bits = [t[b0:b1] for t in outs], self.rate_bits[b0:b1]
                if Bp != n:
                    out = [torch.empty((Bp,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device) for t in outs]
                    bits = torch.zeros(Bp, dtype=torch.float64, device=self.device)
                hipabi.check(fn(self.handle, Bp, T, *([k] if alts else []), _ptr(x), _ptr(c), _ptr(y), _ptr(st),
                                *([_ptr(t) for t in out] or [_ptr(None)]), _ptr(bits), _ptr(self._rate_status), _ptr(ws), ws.numel(),
                                self._stream()), name)
                if not bulk:
                    self._last_forward = (Bp, T, ws)
                if Bp != n:
                    self._unpad_states(b0, b1, st)
                    self.rate_bits[b0:b1] += bits[:n]
                    for whole, part in zip(outs, out):
                        whole[b0:b1] = part[:n]
        return tuple(outs) if alts else (outs[0] if outs else None)

    def rate_window(self, idx, ctx, tgt, want_probs=True):
        """One window of B independent stateful streams as `forward_window` runs it, delivering per position only the
        probability of the target: idx [B,T], ctx [B,T,n_ctx], tgt [B,T] (< 0: no target, probability 0).
        Returns a DEVICE tensor [B,T] f32 (None without want_probs) and adds -log2(max(p, 1e-99)) over each stream's
        valid positions to the f64 accumulator `rate_bits` [B] (rate_bits_read).  Nothing is synchronised here: a timed-out
        scan hand-off surfaces as KlError in rate_bits_read / rate_status_check."""
        return self._rate_call(idx, ctx, tgt, None, False, want_probs)

    def rate_window_bulk(self, idx_d, ctx_d, tgt_d, want_probs=True):
        """`rate_window` on the bf16 training forward (kl_rate_window_bulk): the wide persistent scans take thousands of
        streams per launch.  idx_d [B,T], ctx_d [B,T,n_ctx], tgt_d [B,T]: int32 DEVICE tensors (as `assemble_windows` makes
        them); returns a DEVICE tensor [B,T] f32 (None without want_probs).  Prepares bf16 precision if the handle is in
        another.  Streams are grouped and padded with dummy streams (idx 0, tgt -1, zero state: they deliver nothing and take
        no bits) as `forward_window` does for validation windows.  Bits and status as in `rate_window`."""
        return self._rate_call(idx_d, ctx_d, tgt_d, None, True, want_probs)

    def rate_window_alts(self, idx, ctx, tgt, k):
        """`rate_window` delivering per position also what the model expected instead (kl_rate_window_alts): returns the DEVICE
        tensors tprob [B,T] f32 (what rate_window returns, bit for bit), alt_id [B,T,k] i32 and alt_p [B,T,k] f32 -- the k
        most probable characters, ordered by (logit descending, id ascending), -1 / 0 from the V-th on -- and rank [B,T] i32,
        the target's position in that order (0: the model's first choice; -1 without a target).  Positions with tgt < 0
        deliver 0 / -1 / 0 / -1.  1 <= k <= hipabi.KL_RATE_ALTS_MAX.  Bits go to the same accumulator `rate_bits`, and
        nothing is synchronised here either (rate_bits_read / rate_status_check)."""
        return self._rate_call(idx, ctx, tgt, k, False)

    def rate_window_alts_bulk(self, idx_d, ctx_d, tgt_d, k):
        """`rate_window_alts` on the bf16 training forward (kl_rate_window_alts_bulk): idx_d [B,T], ctx_d [B,T,n_ctx], tgt_d
        [B,T] int32 DEVICE tensors (as `assemble_windows` makes them); returns the DEVICE tensors (tprob [B,T] f32 -- what
        `rate_window_bulk` returns, bit for bit --, alt_id [B,T,k] i32, alt_p [B,T,k] f32, rank [B,T] i32).  Prepares bf16
        precision if the handle is in another; streams are grouped and padded with dummy streams (idx 0, tgt -1, zero state:
        they deliver nothing and take no bits) exactly as `rate_window_bulk` does.  Bits and status as in `rate_window`."""
        return self._rate_call(idx_d, ctx_d, tgt_d, k, True)

    def reset_states_where(self, mask_d):
        """zero the state rows mask_d (bool DEVICE tensor [B]) names: one masked fill, no index list"""
        with self._launch():
            self.states.masked_fill_(mask_d.view(-1, 1, 1), 0.0)

    def rate_scatter(self, tprob, plan, n_ctx, out):
        """kl_rate_scatter: a call's target probabilities tprob [B,T] (f32 DEVICE tensor) to the places of their characters in
        out (f32 DEVICE vector shaped like the id corpus): out[start + 1 + t] = tprob[b][t] for t < min(vlen, T), start and
        vlen from plan (int64 DEVICE tensor [B, 4 + n_ctx], what `assemble_windows` read).  In place, no synchronisation."""
        torch = self.torch
        B, T = int(tprob.shape[0]), int(tprob.shape[1])
        if (tprob.dtype != torch.float32 or out.dtype != torch.float32 or plan.dtype != torch.int64 or plan.dim() != 2
                or tuple(plan.shape) != (B, 4 + n_ctx) or out.dim() != 1
                or not (tprob.is_contiguous() and plan.is_contiguous() and out.is_contiguous())
                or not (tprob.is_cuda and plan.is_cuda and out.is_cuda)):
            raise hipabi.KlError("rate_scatter: tprob f32 [B, T], plan int64 [B, 4 + n_ctx], out f32 [n], contiguous, on the device")
        with self._launch():
            hipabi.check(self.lib.kl_rate_scatter(_ptr(tprob), _ptr(plan), B, T, int(n_ctx), _ptr(out), out.numel(),
                                                  self._stream()), "kl_rate_scatter")
        return out

    def rate_text_bits(self, probs, offsets):
        """kl_rate_text_bits: bits [n] (f64 DEVICE tensor) = per text -sum log2(max(p, 1e-99)) over all but its first character;
        probs f32 DEVICE vector, offsets int64 DEVICE tensor [n + 1], ascending.  No synchronisation."""
        torch = self.torch
        if (probs.dtype != torch.float32 or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2
                or not (probs.is_contiguous() and offsets.is_contiguous()) or not (probs.is_cuda and offsets.is_cuda)):
            raise hipabi.KlError("rate_text_bits: probs f32 [n], offsets int64 [n_texts + 1], contiguous, on the device")
        n = offsets.numel() - 1
        with self._launch():
            bits = torch.empty(n, dtype=torch.float64, device=self.device)
            hipabi.check(self.lib.kl_rate_text_bits(_ptr(probs), _ptr(offsets), n, _ptr(bits), self._stream()),
                         "kl_rate_text_bits")
        return bits

    def rate_scatter_planes(self, tprob, plan, plane, n_ctx, out):
        """kl_rate_scatter_planes: `rate_scatter` with a destination plane per row -- out f32 DEVICE tensor [C, ld], plane int32
        DEVICE tensor [B]: out[plane[b], start + 1 + t] = tprob[b][t] for t < min(vlen, T); a row whose plane is outside
        [0, C) writes nothing.  In place, no synchronisation."""
        torch = self.torch
        B, T = int(tprob.shape[0]), int(tprob.shape[1])
        tensors = (tprob, plan, plane, out)
        if ([t.dtype for t in tensors] != [torch.float32, torch.int64, torch.int32, torch.float32] or plan.dim() != 2
                or tuple(plan.shape) != (B, 4 + n_ctx) or tuple(plane.shape) != (B,) or out.dim() != 2
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("rate_scatter_planes: tprob f32 [B, T], plan int64 [B, 4 + n_ctx], plane int32 [B], out f32 [C, ld], "
                                 "contiguous, on the device")
        C, ld = int(out.shape[0]), int(out.shape[1])
        with self._launch():
            hipabi.check(self.lib.kl_rate_scatter_planes(_ptr(tprob), _ptr(plan), _ptr(plane), B, T, int(n_ctx), C, _ptr(out), ld,
                                                         ld, self._stream()), "kl_rate_scatter_planes")
        return out

    def context_mix(self, planes, offsets, log2prior=None, mix=None):
        """kl_context_mix over planes (f32 DEVICE tensor [C, ld], what `rate_scatter_planes` filled), offsets (int64 DEVICE
        tensor [n + 1]) and log2prior (f64 DEVICE tensor [C], or None: uniform): returns the DEVICE tensors (cand_bits f64
        [n, C], mix_bits f64 [n], post f64 [n, C], best int32 [n], margin f64 [n]); mix (f32 DEVICE tensor [ld], or None)
        takes the mixture's probability at every predicted position, in place.  The statement is ratebulk.context_mix_host.
        No synchronisation."""
        torch = self.torch
        if (planes.dtype != torch.float32 or planes.dim() != 2 or offsets.dtype != torch.int64 or offsets.dim() != 1
                or offsets.numel() < 2 or not (planes.is_contiguous() and offsets.is_contiguous())
                or not (planes.is_cuda and offsets.is_cuda)):
            raise hipabi.KlError("context_mix: planes f32 [C, ld], offsets int64 [n_texts + 1], contiguous, on the device")
        C, ld = int(planes.shape[0]), int(planes.shape[1])
        if log2prior is not None and (log2prior.dtype != torch.float64 or tuple(log2prior.shape) != (C,)
                                      or not (log2prior.is_contiguous() and log2prior.is_cuda)):
            raise hipabi.KlError("context_mix: log2prior f64 [C], contiguous, on the device")
        if mix is not None and (mix.dtype != torch.float32 or tuple(mix.shape) != (ld,)
                                or not (mix.is_contiguous() and mix.is_cuda)):
            raise hipabi.KlError("context_mix: mix f32 [ld], contiguous, on the device")
        n = offsets.numel() - 1
        with self._launch():
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
            cand_bits, mix_bits, post, margin = f64(n, C), f64(n), f64(n, C), f64(n)
            best = torch.empty(n, dtype=torch.int32, device=self.device)
            hipabi.check(self.lib.kl_context_mix(_ptr(planes), ld, _ptr(offsets), n, C, _ptr(log2prior), _ptr(mix),
                                                 _ptr(cand_bits), _ptr(mix_bits), _ptr(post), _ptr(best), _ptr(margin),
                                                 self._stream()), "kl_context_mix")
        return cand_bits, mix_bits, post, best, margin

    def rate_scatter_alts(self, tprob, rank, alt_id, alt_p, plan, n_ctx, out_prob, out_rank, out_alt_id, out_alt_p):
        """kl_rate_scatter_alts: `rate_scatter` for all four results of a `rate_window_alts(_bulk)` call (DEVICE tensors tprob,
        rank [B,T], alt_id, alt_p [B,T,k]) into corpus-order DEVICE arrays out_prob f32 [n], out_rank i32 [n], out_alt_id i32
        [n,k], out_alt_p f32 [n,k]: position start + 1 + t takes [b][t] for t < min(vlen, T), start and vlen from plan (int64
        DEVICE tensor [B, 4 + n_ctx]).  In place, no synchronisation."""
        torch = self.torch
        B, T = int(tprob.shape[0]), int(tprob.shape[1])
        k = int(alt_id.shape[-1])
        n = out_prob.numel()
        tensors = (tprob, rank, alt_id, alt_p, plan, out_prob, out_rank, out_alt_id, out_alt_p)
        if ([t.dtype for t in tensors] != [torch.float32, torch.int32, torch.int32, torch.float32, torch.int64, torch.float32,
                                           torch.int32, torch.int32, torch.float32]
                or tuple(rank.shape) != (B, T) or tuple(alt_id.shape) != (B, T, k) or tuple(alt_p.shape) != (B, T, k)
                or plan.dim() != 2 or tuple(plan.shape) != (B, 4 + n_ctx) or out_prob.dim() != 1
                or tuple(out_rank.shape) != (n,) or tuple(out_alt_id.shape) != (n, k) or tuple(out_alt_p.shape) != (n, k)
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("rate_scatter_alts: tprob f32 / rank i32 [B, T], alt_id i32 / alt_p f32 [B, T, k], plan int64 "
                                 "[B, 4 + n_ctx], out_prob f32 / out_rank i32 [n], out_alt_id i32 / out_alt_p f32 [n, k], "
                                 "contiguous, on the device")
        with self._launch():
            hipabi.check(self.lib.kl_rate_scatter_alts(
                _ptr(tprob), _ptr(rank), _ptr(alt_id), _ptr(alt_p), _ptr(plan), B, T, k, int(n_ctx), _ptr(out_prob),
                _ptr(out_rank), _ptr(out_alt_id), _ptr(out_alt_p), n, self._stream()), "kl_rate_scatter_alts")

    def rate_select(self, probs, rank, alt_id, alt_p, max_prob, min_rank):
        """kl_rate_select over corpus-order DEVICE arrays (probs f32 [n], rank i32 [n], alt_id i32 [n,k], alt_p f32 [n,k]): the
        positions j with rank[j] >= min_rank and probs[j] <= float32(max_prob), ascending, as DEVICE tensors (pos i64 [m], prob
        f32 [m], rank i32 [m], alt_id i32 [m,k], alt_p f32 [m,k]).  One counting call, one read of the count -- the only
        wait --, buffers of exactly that size, one writing call; nothing more is launched when the count is 0."""
        torch = self.torch
        n = probs.numel()
        k = int(alt_id.shape[-1]) if alt_id.dim() == 2 else 0
        tensors = (probs, rank, alt_id, alt_p)
        if ([t.dtype for t in tensors] != [torch.float32, torch.int32, torch.int32, torch.float32] or probs.dim() != 1
                or tuple(rank.shape) != (n,) or tuple(alt_id.shape) != (n, k) or tuple(alt_p.shape) != (n, k)
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("rate_select: probs f32 / rank i32 [n], alt_id i32 / alt_p f32 [n, k], contiguous, on the device")
        min_rank = int(min_rank)
        max_prob = float(np.float32(max_prob))
        if min_rank < 0 or max_prob != max_prob:
            raise ValueError("rate_select: min_rank >= 0 and max_prob not NaN")
        dev = self.device
        empty = lambda m: (torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.float32, device=dev),
                           torch.empty(m, dtype=torch.int32, device=dev), torch.empty((m, k), dtype=torch.int32, device=dev),
                           torch.empty((m, k), dtype=torch.float32, device=dev))
        if n == 0:
            return empty(0)
        with self._launch():
            n_ws = self.lib.kl_rate_select_workspace_bytes(n)
            if self._rate_select_ws is None or self._rate_select_ws.numel() < n_ws:
                self._rate_select_ws = None
                self._rate_select_ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
            ws = self._rate_select_ws
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            call = lambda m, out: hipabi.check(self.lib.kl_rate_select(
                _ptr(probs), _ptr(rank), _ptr(alt_id), _ptr(alt_p), n, k, max_prob, min_rank, m, _ptr(out[0]), _ptr(out[1]),
                _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(count), _ptr(ws), ws.numel(), self._stream()), "kl_rate_select")
            call(0, (None,) * 5)
            m = int(count.item())
            out = empty(m)
            if m:
                call(m, out)
        return out

    def _scratch(self, slot, n_bytes):
        """the device scratch kept on the engine under `slot`, grown to n_bytes"""
        ws = getattr(self, slot)
        if ws is None or ws.numel() < n_bytes:
            setattr(self, slot, None)
            ws = self.torch.empty(max(n_bytes, 8), dtype=self.torch.uint8, device=self.device)
            setattr(self, slot, ws)
        return ws

    def word_bounds(self, corpus_d, offsets_d, delim_d):
        """kl_word_bounds over corpus_d int32 [n] and offsets_d int64 [n_texts + 1] as bulk rating keeps them and delim_d uint8
        [V] (nonzero: the id separates words) -- DEVICE tensors: the words of the texts as DEVICE tensors (start int64 [m], end
        int64 [m]), ascending, [start, end) in corpus positions; the statement is ratebulk.word_bounds_host.  One counting call,
        one read of the count -- the only wait --, buffers of exactly that size, one writing call; nothing more is launched
        when the count is 0."""
        torch = self.torch
        tensors = (corpus_d, offsets_d, delim_d)
        if ([t.dtype for t in tensors] != [torch.int32, torch.int64, torch.uint8] or any(t.dim() != 1 for t in tensors)
                or offsets_d.numel() < 2 or delim_d.numel() < 1 or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("word_bounds: corpus int32 [n], offsets int64 [n_texts + 1], delim uint8 [V], contiguous, on the "
                                 "device")
        dev = self.device
        n, n_texts, V = corpus_d.numel(), offsets_d.numel() - 1, delim_d.numel()
        empty = lambda m: (torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int64, device=dev))
        if n == 0:
            return empty(0)
        with self._launch():
            ws = self._scratch("_word_bounds_ws", self.lib.kl_word_bounds_workspace_bytes(n, n_texts))
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            call = lambda m, out: hipabi.check(self.lib.kl_word_bounds(
                _ptr(corpus_d), n, _ptr(offsets_d), n_texts, _ptr(delim_d), V, m, _ptr(out[0]), _ptr(out[1]), _ptr(count),
                _ptr(ws), ws.numel(), self._stream()), "kl_word_bounds")
            call(0, (None, None))
            m = int(count.item())
            out = empty(m)
            if m:
                call(m, out)
        return out

    def rate_segments(self, probs, rank, offsets_d, seg_start, seg_end, max_prob=0.0, min_rank=0):
        """kl_rate_segments over corpus-order DEVICE arrays probs f32 [n] and rank int32 [n] (None: no suspects are counted),
        offsets_d int64 [n_texts + 1] and the segments seg_start, seg_end int64 [S] (any order, overlap allowed): the DEVICE
        tensors (n int32, bits f64, psum f64, min f32, worst int64, bad int32), each [S]; the statement is
        ratebulk.segments_host.  No synchronisation."""
        torch = self.torch
        tensors = [probs, offsets_d, seg_start, seg_end] + ([rank] if rank is not None else [])
        kinds = [torch.float32, torch.int64, torch.int64, torch.int64] + ([torch.int32] if rank is not None else [])
        n, S = probs.numel(), seg_start.numel()
        if ([t.dtype for t in tensors] != kinds or any(t.dim() != 1 for t in tensors) or offsets_d.numel() < 2
                or seg_end.numel() != S or (rank is not None and rank.numel() != n)
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("rate_segments: probs f32 / rank int32 [n], offsets int64 [n_texts + 1], seg_start / seg_end int64 "
                                 "[S], contiguous, on the device")
        min_rank = int(min_rank)
        max_prob = float(np.float32(max_prob))
        if min_rank < 0 or max_prob != max_prob:
            raise ValueError("rate_segments: min_rank >= 0 and max_prob not NaN")
        dev = self.device
        with self._launch():
            out = tuple(torch.empty(S, dtype=kind, device=dev)
                        for kind in (torch.int32, torch.float64, torch.float64, torch.float32, torch.int64, torch.int32))
            if S:
                hipabi.check(self.lib.kl_rate_segments(
                    _ptr(probs), _ptr(rank), n, _ptr(offsets_d), offsets_d.numel() - 1, _ptr(seg_start), _ptr(seg_end), S, max_prob,
                    min_rank, *([_ptr(t) for t in out] + [self._stream()])), "kl_rate_segments")
        return out

    def segment_select(self, seg_start, seg_end, records, min_n=1, min_bad=1, min_bpc=0.0):
        """kl_segment_select over seg_start, seg_end int64 [S] and the records `rate_segments` returned (DEVICE tensors): the
        segments with n >= min_n, bad >= min_bad and bits >= min_bpc * n, ascending, as DEVICE tensors (index int64 [m], start,
        end, n, bits, psum, min, worst, bad -- bit copies of the records); the statement is ratebulk.segment_select_host.  One
        counting call, one read of the count -- the only wait --, buffers of exactly that size, one writing call; nothing more
        is launched when the count is 0."""
        torch = self.torch
        src = (seg_start, seg_end) + tuple(records)
        kinds = [torch.int64, torch.int64, torch.int32, torch.float64, torch.float64, torch.float32, torch.int64, torch.int32]
        S = seg_start.numel()
        if (len(src) != 8 or [t.dtype for t in src] != kinds or any(tuple(t.shape) != (S,) for t in src)
                or not all(t.is_contiguous() and t.is_cuda for t in src)):
            raise hipabi.KlError("segment_select: seg_start / seg_end int64 and the six records of rate_segments, [S] each, "
                                 "contiguous, on the device")
        min_n, min_bad, min_bpc = int(min_n), int(min_bad), float(min_bpc)
        if min_n < 1 or min_bad < 0 or not min_bpc >= 0.0:
            raise ValueError("segment_select: min_n >= 1, min_bad >= 0 and min_bpc >= 0, not NaN")
        dev = self.device
        empty = lambda m: tuple(torch.empty(m, dtype=kind, device=dev) for kind in [torch.int64] + kinds)
        if S == 0:
            return empty(0)
        with self._launch():
            ws = self._scratch("_segment_select_ws", self.lib.kl_segment_select_workspace_bytes(S))
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            call = lambda m, out: hipabi.check(self.lib.kl_segment_select(
                *([_ptr(t) for t in src] + [S, min_n, min_bad, min_bpc, m] + [_ptr(t) for t in out]
                  + [_ptr(count), _ptr(ws), ws.numel(), self._stream()])), "kl_segment_select")
            call(0, (None,) * 9)
            m = int(count.item())
            out = empty(m)
            if m:
                call(m, out)
        return out

    def _lexicon_fits(self, method, chars_d, order_d, class_first, q_pool_d, q_off_d):
        """What `lexicon_neighbours`, `lexicon_splits`, `lexicon_chains` and `lexicon_channel` ask of the lexicon and the queries
        before anything else, hipabi.KlError with `method` in front otherwise: chars_d, order_d, q_pool_d int32 and q_off_d int64
        [Q + 1], of one dimension, contiguous, on the device; class_first int64 [66] on the host.  Returns class_first as a
        contiguous array and Q."""
        torch = self.torch
        tensors = (chars_d, order_d, q_pool_d, q_off_d)
        if ([t.dtype for t in tensors] != [torch.int32, torch.int32, torch.int32, torch.int64] or any(t.dim() != 1 for t in tensors)
                or q_off_d.numel() < 2 or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("%s: chars, order and q_pool int32, q_off int64 [Q + 1], contiguous, on the device" % method)
        class_first = np.ascontiguousarray(class_first, dtype=np.int64).reshape(-1)
        if len(class_first) != 66 or order_d.numel() != int(class_first[-1]):
            raise hipabi.KlError("%s: class_first int64 [66] on the host, its last value the size of order" % method)
        return class_first, q_off_d.numel() - 1

    def _lexicon_call(self, entry, ws_name, ws_bytes, lexicon_args, middle, shapes):
        """The launch of the four lexicon look-ups: allocates int32 outputs of `shapes`, takes the scratch kept under ws_name at
        ws_bytes, and calls `entry` with the nine arguments lexicon_args stands for (chars_d, order_d, class_first, V, q_pool_d,
        q_off_d and the sizes), then middle (the entry point's own), then the outputs, the workspace and the stream.  Returns
        the DEVICE tensors."""
        torch = self.torch
        chars_d, order_d, class_first, V, q_pool_d, q_off_d = lexicon_args
        with self._launch():
            ws = self._scratch(ws_name, ws_bytes)
            out = tuple(torch.empty(shape, dtype=torch.int32, device=self.device) for shape in shapes)
            hipabi.check(entry(
                _ptr(chars_d), chars_d.numel(), _ptr(order_d), class_first.ctypes.data, V, _ptr(q_pool_d), q_pool_d.numel(),
                _ptr(q_off_d), q_off_d.numel() - 1, *middle, *([_ptr(t) for t in out] + [_ptr(ws), ws.numel(), self._stream()])),
                entry.__name__)
        return out

    def lexicon_neighbours(self, chars_d, order_d, class_first, V, q_pool_d, q_off_d, max_dist, K):
        """kl_lexicon_neighbours: the entries of a lexicon within max_dist edits of Q query words.  chars_d int32 and order_d
        int32 [N'] are DEVICE copies of what `ratebulk.lexicon_layout_host` built, class_first its int64 [66] on the HOST (every
        bound is checked there before the launch); q_pool_d int32 and q_off_d int64 [Q + 1] the queries on the DEVICE; ids are
        equal only within [0, V).  Returns the DEVICE tensors (exact int32 [Q], found int32 [Q], cand int32 [Q, K], dist int32
        [Q, K]); the statement is ratebulk.lexicon_neighbours_host.  hipabi.KlError for what the entry point rejects.  No
        synchronisation."""
        class_first, Q = self._lexicon_fits("lexicon_neighbours", chars_d, order_d, class_first, q_pool_d, q_off_d)
        V, max_dist, K = int(V), int(max_dist), int(K)
        return self._lexicon_call(self.lib.kl_lexicon_neighbours, "_lexicon_ws",
                                  self.lib.kl_lexicon_neighbours_workspace_bytes(Q, K),
                                  (chars_d, order_d, class_first, V, q_pool_d, q_off_d), (max_dist, K),
                                  [Q, Q, (Q, max(K, 0)), (Q, max(K, 0))])

    def lexicon_splits(self, chars_d, order_d, class_first, V, q_pool_d, q_off_d, max_dist, min_part, K):
        """kl_lexicon_splits: the places at which Q query words fall into two entries of a lexicon, a lost delimiter counted as
        one of max_dist edits and every half of at least min_part ids.  The lexicon, V and the queries as in
        `lexicon_neighbours`.  Returns the DEVICE tensors (found int32 [Q], split, left, right, dist int32 [Q, K]); the statement
        is ratebulk.lexicon_splits_host.  hipabi.KlError for what the entry point rejects.  No synchronisation."""
        class_first, Q = self._lexicon_fits("lexicon_splits", chars_d, order_d, class_first, q_pool_d, q_off_d)
        V, max_dist, min_part, K = int(V), int(max_dist), int(min_part), int(K)
        return self._lexicon_call(self.lib.kl_lexicon_splits, "_lexicon_splits_ws",
                                  self.lib.kl_lexicon_splits_workspace_bytes(Q, K),
                                  (chars_d, order_d, class_first, V, q_pool_d, q_off_d), (max_dist, min_part, K),
                                  [Q] + [(Q, max(K, 0))] * 4)

    def lexicon_chains(self, chars_d, order_d, class_first, V, q_pool_d, q_off_d, links, max_parts, min_part):
        """kl_lexicon_chains: Q query words as chains of up to P = max_parts exact entries of a lexicon, every piece of at
        least min_part ids, with the linking elements `links` allowed between pieces -- a sequence of id sequences (1 .. 3 ids
        each, at most 8) or the int32 [n, 4] of `ratebulk.lexicon_links_host`, read on the HOST.  The lexicon, V and the
        queries as in `lexicon_neighbours`.  Returns the DEVICE tensors (found int32 [Q], worst int32 [Q, P], entry, start,
        link int32 [Q, P, P]); the statement is ratebulk.lexicon_chains_host.  hipabi.KlError for what the entry point
        rejects.  No synchronisation."""
        class_first, Q = self._lexicon_fits("lexicon_chains", chars_d, order_d, class_first, q_pool_d, q_off_d)
        V, P, min_part = int(V), int(max_parts), int(min_part)
        try:
            links = np.ascontiguousarray(ratebulk.lexicon_links_host(links, V), dtype=np.int32)
        except ValueError as err:
            raise hipabi.KlError(str(err))
        room = min(max(P, 0), hipabi.KL_LEXICON_PARTS_MAX)      # (an out-of-range P is the entry point's to refuse)
        return self._lexicon_call(self.lib.kl_lexicon_chains, "_lexicon_chains_ws",
                                  self.lib.kl_lexicon_chains_workspace_bytes(Q, P),
                                  (chars_d, order_d, class_first, V, q_pool_d, q_off_d),
                                  (links.ctypes.data if len(links) else None, len(links), P, min_part),
                                  [Q, (Q, room)] + [(Q, room, room)] * 3)

    def lexicon_channel(self, chars_d, order_d, class_first, V, q_pool_d, q_off_d, rules_d, rule_cost_d, unit, max_cost, K):
        """kl_lexicon_channel: the entries of a lexicon within max_cost of Q query words in the weighted distance of a
        confusion table.  The lexicon, V and the queries as in `lexicon_neighbours`; rules_d int32 [R, 10] (src_len, tgt_len,
        src[4], tgt[4]: the source stands in the query) and rule_cost_d int32 [R] on the DEVICE, both None for no rules;
        unit the cost of a plain edit.  Returns the DEVICE tensors (exact int32 [Q], found int32 [Q], cand int32 [Q, K], cost
        int32 [Q, K]); the statement is ratebulk.lexicon_channel_host.  hipabi.KlError for what the entry point rejects.  No
        synchronisation."""
        torch = self.torch
        class_first, Q = self._lexicon_fits("lexicon_channel", chars_d, order_d, class_first, q_pool_d, q_off_d)
        R = 0
        if rules_d is not None or rule_cost_d is not None:
            both = (rules_d, rule_cost_d)
            if (any(t is None or t.dtype != torch.int32 or not (t.is_contiguous() and t.is_cuda) for t in both)
                    or rules_d.dim() != 2 or rules_d.shape[1] != 10 or rule_cost_d.dim() != 1
                    or rule_cost_d.numel() != rules_d.shape[0]):
                raise hipabi.KlError("lexicon_channel: rules int32 [R, 10] and rule_cost int32 [R], contiguous, on the device")
            R = int(rule_cost_d.numel())
        V, unit, max_cost, K = int(V), int(unit), int(max_cost), int(K)
        return self._lexicon_call(self.lib.kl_lexicon_channel, "_lexicon_channel_ws",
                                  self.lib.kl_lexicon_channel_workspace_bytes(Q, K, R),
                                  (chars_d, order_d, class_first, V, q_pool_d, q_off_d),
                                  (_ptr(rules_d) if R else None, _ptr(rule_cost_d) if R else None, R, unit, max_cost, K),
                                  [Q, Q, (Q, max(K, 0)), (Q, max(K, 0))])

    def _hypothesis_fits(self, source, own):
        """Whether the tensors of `variant_windows`, `prefix_windows` or `span_windows` are as the call's message says:
        source (corpus_d int32 [n], offsets_d int64 [n_texts + 1], text_ctx_d int32 [n_texts, n_ctx] or None) and own, the
        call's further tensors as (tensor, dtype, dims), every one contiguous and on the device.  The sizes of `own` against
        each other are the call's to compare."""
        torch = self.torch
        corpus_d, offsets_d, text_ctx_d = source
        told = [(corpus_d, torch.int32, 1), (offsets_d, torch.int64, 1)] + own
        contexts = text_ctx_d is not None and text_ctx_d.shape[-1] > 0
        if contexts:
            told.append((text_ctx_d, torch.int32, 2))
        return (all(t is not None and t.dtype == kind and t.dim() == dims and t.is_contiguous() and t.is_cuda
                    for t, kind, dims in told)
                and (not contexts or text_ctx_d.shape[0] == offsets_d.numel() - 1))

    def _hypothesis_rows(self, entry, source, rows, T, middle):
        """The launch of `variant_windows`, `prefix_windows` and `span_windows`: allocates the four outputs and calls `entry`
        with the six arguments of source (corpus_d, offsets_d, text_ctx_d), then middle (the entry point's own), then T, the
        outputs and the stream.  Returns the DEVICE tensors (idx [rows, T], ctx [rows, T, n_ctx], tgt [rows, T], valid [rows])
        int32."""
        torch = self.torch
        corpus_d, offsets_d, text_ctx_d = source
        n_ctx = 0 if text_ctx_d is None else int(text_ctx_d.shape[-1])
        with self._launch():
            idx = torch.empty((rows, T), dtype=torch.int32, device=self.device)
            tgt = torch.empty((rows, T), dtype=torch.int32, device=self.device)
            ctx = torch.empty((rows, T, n_ctx), dtype=torch.int32, device=self.device)
            valid = torch.empty(rows, dtype=torch.int32, device=self.device)
            hipabi.check(entry(
                _ptr(corpus_d), corpus_d.numel(), _ptr(offsets_d), offsets_d.numel() - 1, _ptr(text_ctx_d) if n_ctx else None,
                n_ctx, *middle, T, _ptr(idx), _ptr(ctx) if n_ctx else None, _ptr(tgt), _ptr(valid), self._stream()),
                entry.__name__)
        return idx, ctx, tgt, valid

    def align_pairs(self, a_pool_d, a_off_d, b_pool_d, b_off_d, max_len, max_dist, join):
        """kl_align_pairs: where the texts of P pairs differ, within a band of max_dist edits.  a_pool_d, b_pool_d int32 symbols
        and a_off_d, b_off_d int64 [P + 1] on the DEVICE: text p of a side is pool[off[p]:off[p + 1]].  Returns the DEVICE tensors
        (dist int32 [P], n_spans int32 [P], spans int32 [P, max_dist, 4]); the statement is ratebulk.align_pairs_host.
        hipabi.KlError for what the entry point rejects.  No synchronisation."""
        torch = self.torch
        tensors = (a_pool_d, a_off_d, b_pool_d, b_off_d)
        if ([t.dtype for t in tensors] != [torch.int32, torch.int64, torch.int32, torch.int64] or any(t.dim() != 1 for t in tensors)
                or a_off_d.numel() < 2 or a_off_d.numel() != b_off_d.numel()
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("align_pairs: pools int32, offsets int64 [P + 1] of one size, contiguous, on the device")
        max_len, max_dist, join = int(max_len), int(max_dist), int(join)
        P = a_off_d.numel() - 1
        dev = self.device
        with self._launch():
            ws = self._scratch("_align_ws", self.lib.kl_align_pairs_workspace_bytes(P, max_len, max_dist))
            out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                   torch.empty((P, max(max_dist, 0), 4), dtype=torch.int32, device=dev))
            hipabi.check(self.lib.kl_align_pairs(
                _ptr(a_pool_d), a_pool_d.numel(), _ptr(a_off_d), _ptr(b_pool_d), b_pool_d.numel(), _ptr(b_off_d), P, max_len,
                max_dist, join, *([_ptr(t) for t in out] + [_ptr(ws), ws.numel(), self._stream()])), "kl_align_pairs")
        return out

    def confusion_counts(self, a_pool_d, a_off_d, b_pool_d, b_off_d, dist_d, n_spans_d, spans_d, max_chars, room):
        """kl_confusion_counts: the table of confusions the spans of `align_pairs` amount to (a the OCR, b the truth).  The
        texts as `align_pairs` took them and the three tensors it returned, all on the DEVICE.  Returns the DEVICE tensors
        (rules int32 [room, 10], count int64 [room], occ int64 [room], stats int64 [4]); the statement is
        ratebulk.confusion_counts_host.  hipabi.KlError for what the entry point rejects.  No synchronisation."""
        torch = self.torch
        tensors = (a_pool_d, a_off_d, b_pool_d, b_off_d, dist_d, n_spans_d, spans_d)
        P = a_off_d.numel() - 1
        if ([t.dtype for t in tensors] != [torch.int32, torch.int64, torch.int32, torch.int64] + [torch.int32] * 3
                or any(t.dim() != 1 for t in tensors[:6]) or P < 1 or b_off_d.numel() != P + 1 or dist_d.numel() != P
                or n_spans_d.numel() != P or spans_d.dim() != 3 or spans_d.shape[0] != P or spans_d.shape[2] != 4
                or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("confusion_counts: pools int32, offsets int64 [P + 1], dist and n_spans int32 [P], spans int32 "
                                 "[P, max_dist, 4], contiguous, on the device")
        max_chars, room, max_dist = int(max_chars), int(room), int(spans_d.shape[1])
        dev = self.device
        with self._launch():
            ws = self._scratch("_confusion_ws", self.lib.kl_confusion_counts_workspace_bytes(P, max_dist, a_pool_d.numel()))
            rows = max(room, 0)
            out = (torch.empty((rows, 10), dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int64, device=dev),
                   torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev))
            hipabi.check(self.lib.kl_confusion_counts(
                _ptr(a_pool_d), a_pool_d.numel(), _ptr(a_off_d), _ptr(b_pool_d), b_pool_d.numel(), _ptr(b_off_d), P, max_dist,
                _ptr(dist_d), _ptr(n_spans_d), _ptr(spans_d), max_chars, rows,
                *([_ptr(t) for t in out] + [_ptr(ws), ws.numel(), self._stream()])), "kl_confusion_counts")
        return out

    def witness_clusters(self, b_pool_d, b_off_d, dist_d, n_spans_d, spans_d, pair_first_d, text_off_d, join):
        """kl_witness_clusters: the differing spans of all witnesses of a text clustered, the witnesses' readings of every
        cluster made distinct and counted.  Side b as `align_pairs` took it and the three tensors it returned, pair_first_d and
        text_off_d int64 [n_texts + 1] (the pairs of every text; the texts' offsets in `span_windows`' corpus), all on the
        DEVICE.  With R = P * max_dist returns the DEVICE tensors (span_text int32 [R], span_start int64 [R], span_len int32
        [R], span_first int64 [R + 1], cand_src int64 [R], cand_off int64 [R + 1], votes int32 [2 R], stats int64 [8]); the
        statement is ratebulk.witness_clusters_host.  hipabi.KlError for what the entry point rejects.  No synchronisation."""
        torch = self.torch
        tensors = (b_pool_d, b_off_d, dist_d, n_spans_d, spans_d, pair_first_d, text_off_d)
        P = b_off_d.numel() - 1
        if ([t.dtype for t in tensors] != [torch.int32, torch.int64] + [torch.int32] * 3 + [torch.int64] * 2
                or any(t.dim() != 1 for t in tensors[:4] + tensors[5:]) or P < 1 or dist_d.numel() != P or n_spans_d.numel() != P
                or spans_d.dim() != 3 or spans_d.shape[0] != P or spans_d.shape[2] != 4 or pair_first_d.numel() < 2
                or text_off_d.numel() != pair_first_d.numel() or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("witness_clusters: b_pool int32, b_off int64 [P + 1], dist and n_spans int32 [P], spans int32 "
                                 "[P, max_dist, 4], pair_first and text_off int64 [n_texts + 1], contiguous, on the device")
        max_dist, join, n_texts = int(spans_d.shape[1]), int(join), pair_first_d.numel() - 1
        R = P * max_dist
        dev, i32, i64 = self.device, torch.int32, torch.int64
        with self._launch():
            ws = self._scratch("_witness_ws", self.lib.kl_witness_clusters_workspace_bytes(P, max_dist, n_texts))
            out = tuple(torch.empty(n, dtype=kind, device=dev)
                        for n, kind in ((R, i32), (R, i64), (R, i32), (R + 1, i64), (R, i64), (R + 1, i64), (2 * R, i32), (8, i64)))
            hipabi.check(self.lib.kl_witness_clusters(
                _ptr(b_pool_d), b_pool_d.numel(), _ptr(b_off_d), P, max_dist, _ptr(dist_d), _ptr(n_spans_d), _ptr(spans_d),
                _ptr(pair_first_d), _ptr(text_off_d), n_texts, join,
                *([_ptr(t) for t in out] + [_ptr(ws), ws.numel(), self._stream()])), "kl_witness_clusters")
        return out

    def witness_pool(self, b_ids_d, cand_src_d, cand_off_d, C, n_pool):
        """kl_witness_pool: the C candidates of `witness_clusters` as ids -- pool[cand_off[c] + k] = b_ids[cand_src[c] + k].
        b_ids_d int32 [n_b] (the witnesses encoded with the rater's mapping, parallel to b_pool), cand_src_d int64 (at least C)
        and cand_off_d int64 (at least C + 1) on the DEVICE; C and n_pool as `witness_clusters`' stats gave them.  Returns the
        DEVICE tensor pool int32 [n_pool]: what ratebulk.witness_pool_host states.  No synchronisation."""
        torch = self.torch
        tensors = (b_ids_d, cand_src_d, cand_off_d)
        C, n_pool = int(C), int(n_pool)
        if ([t.dtype for t in tensors] != [torch.int32, torch.int64, torch.int64] or any(t.dim() != 1 for t in tensors)
                or not all(t.is_contiguous() and t.is_cuda for t in tensors) or C < 1 or n_pool < 0
                or cand_src_d.numel() < C or cand_off_d.numel() < C + 1):
            raise hipabi.KlError("witness_pool: b_ids int32, cand_src int64 [C ..], cand_off int64 [C + 1 ..], contiguous, on the "
                                 "device, C >= 1, n_pool >= 0")
        with self._launch():
            pool = torch.empty(n_pool, dtype=torch.int32, device=self.device)
            hipabi.check(self.lib.kl_witness_pool(_ptr(b_ids_d) if b_ids_d.numel() else None, b_ids_d.numel(), _ptr(cand_src_d),
                                                  _ptr(cand_off_d), C, _ptr(pool) if n_pool else None, n_pool, self._stream()),
                         "kl_witness_pool")
        return pool

    def variant_windows(self, corpus_d, offsets_d, text_ctx_d, sel_pos_d, sel_alt_id_d, left, ahead, deletions, T,
                        insertions=False):
        """kl_edit_windows (kl_variant_windows with insertion rows): the hypothesis rows of S suspects, built on the device in one launch.  corpus_d int32 [n] and
        offsets_d int64 [n_texts + 1] as bulk rating keeps them, text_ctx_d int32 [n_texts, n_ctx] (None without contexts),
        sel_pos_d int64 [S] and sel_alt_id_d int32 [S, K] as `rate_select` returns them (or slices of them) -- all DEVICE
        tensors.  Returns the DEVICE tensors (idx [S*R, T], ctx [S*R, T, n_ctx], tgt [S*R, T], valid [S*R]) int32 with
        R = K + 1 + deletions + K * insertions, row s * R + v: what `ratebulk.variant_windows_host` states (insertions: every
        alternative once more, in front of the written character; T >= left + ahead + 1 then).  hipabi.KlError for what the
        entry point rejects.  No synchronisation."""
        source, torch = (corpus_d, offsets_d, text_ctx_d), self.torch
        if (not self._hypothesis_fits(source, [(sel_pos_d, torch.int64, 1), (sel_alt_id_d, torch.int32, 2)])
                or sel_alt_id_d.shape[0] != sel_pos_d.numel()):
            raise hipabi.KlError(_HYPOTHESIS_TENSORS % ("variant_windows", "sel_pos int64 [S], sel_alt_id int32 [S, K]"))
        S, K = sel_alt_id_d.shape
        left, ahead, deletions, T, insertions = int(left), int(ahead), int(bool(deletions)), int(T), int(insertions)
        if insertions not in (0, 1):
            raise hipabi.KlError("variant_windows: insertions is a flag (got %d)" % insertions)
        return self._hypothesis_rows(self.lib.kl_edit_windows, source, S * (K + 1 + deletions + K * insertions), T,
                                     (_ptr(sel_pos_d), _ptr(sel_alt_id_d), S, K, left, ahead, deletions, insertions))

    def prefix_windows(self, corpus_d, offsets_d, text_ctx_d, sel_pos_d, left, T):
        """kl_prefix_windows: the left context of S suspects as rows of their own, one per suspect, built on the device in one
        launch.  corpus_d int32 [n], offsets_d int64 [n_texts + 1], text_ctx_d int32 [n_texts, n_ctx] (None without contexts)
        and sel_pos_d int64 [S] (or a slice) as in `variant_windows` -- all DEVICE tensors.  Returns the DEVICE tensors (idx
        [S, T], ctx [S, T, n_ctx], tgt [S, T], valid [S]) int32: what `ratebulk.prefix_windows_host` states.  hipabi.KlError for
        what the entry point rejects.  No synchronisation."""
        source = (corpus_d, offsets_d, text_ctx_d)
        if not self._hypothesis_fits(source, [(sel_pos_d, self.torch.int64, 1)]):
            raise hipabi.KlError(_HYPOTHESIS_TENSORS % ("prefix_windows", "sel_pos int64 [S]"))
        S, left, T = int(sel_pos_d.numel()), int(left), int(T)
        if S < 1 or T < 1:
            raise hipabi.KlError("prefix_windows: S >= 1, T >= 1 (got %d, %d)" % (S, T))
        return self._hypothesis_rows(self.lib.kl_prefix_windows, source, S, T, (_ptr(sel_pos_d), S, left))

    def fan_states(self, src_states, parent_d):
        """kl_state_fanout: the states of the streams that continue from the rows of src_states (f32 DEVICE tensor [n, 2 depth,
        pwidth], as `states` is after a window) -- stream b from row parent_d[b] (int32 DEVICE tensor [rows]), from a zero state
        where that names no row: what `ratebulk.fan_states_host` states.  The result is installed as `states` and returned.  It
        lives in a buffer the engine keeps per number of rows (a window's replayed launch sequence is keyed by the address of its
        states), another one where src_states is that buffer itself.  hipabi.KlError for what the entry point rejects.  No
        synchronisation."""
        torch = self.torch
        shape = (2 * self.depth, self.pwidth)
        if (not isinstance(src_states, torch.Tensor) or not isinstance(parent_d, torch.Tensor) or src_states.dtype != torch.float32
                or parent_d.dtype != torch.int32 or src_states.dim() != 3 or tuple(src_states.shape[1:]) != shape
                or parent_d.dim() != 1 or src_states.shape[0] < 1 or parent_d.numel() < 1
                or not all(t.is_contiguous() and t.is_cuda for t in (src_states, parent_d))):
            raise hipabi.KlError("fan_states: states f32 [n, %d, %d] and parent int32 [rows], contiguous, on the device" % shape)
        rows = int(parent_d.numel())
        row_bytes = 4 * shape[0] * shape[1]
        with self._launch():
            dst = self._fan_states.get(rows)
            if dst is not None:      # (disjoint from the source?  a slice of the buffer counts as the buffer)
                a, b = dst.data_ptr(), src_states.data_ptr()
                if a < b + src_states.shape[0] * row_bytes and b < a + rows * row_bytes:
                    dst = None
            if dst is None:
                dst = self._fan_states[rows] = torch.empty((rows,) + shape, dtype=torch.float32, device=self.device)
            hipabi.check(self.lib.kl_state_fanout(_ptr(src_states), int(src_states.shape[0]), _ptr(parent_d), rows,
                                                  shape[0] * shape[1], _ptr(dst), self._stream()), "kl_state_fanout")
        self.states = dst
        return dst

    def span_windows(self, corpus_d, offsets_d, text_ctx_d, span_text_d, span_start_d, span_len_d, span_first_d, pool_d,
                     cand_off_d, row0, rows, left, ahead, max_len, T):
        """kl_span_windows: hypothesis rows row0 .. row0 + rows - 1 of S spans with caller-supplied replacements, built on the
        device in one launch.  corpus_d int32 [n], offsets_d int64 [n_texts + 1] and text_ctx_d int32 [n_texts, n_ctx] (None
        without contexts) as in `variant_windows`; span_text_d int32 [S], span_start_d int64 [S], span_len_d int32 [S],
        span_first_d int64 [S + 1], pool_d int32 [n_pool] and cand_off_d int64 [C + 1] -- all DEVICE tensors; S + C is the
        number of rows there are.  Returns the DEVICE tensors (idx [rows, T], ctx [rows, T, n_ctx], tgt [rows, T], valid
        [rows]) int32: what `ratebulk.span_windows_host` states.  hipabi.KlError for what the entry point rejects.  No
        synchronisation (span_first_d[S] == C is the caller's word)."""
        source, i32, i64 = (corpus_d, offsets_d, text_ctx_d), self.torch.int32, self.torch.int64
        if (not self._hypothesis_fits(source, [(span_text_d, i32, 1), (span_start_d, i64, 1), (span_len_d, i32, 1),
                                               (span_first_d, i64, 1), (pool_d, i32, 1), (cand_off_d, i64, 1)])
                or span_first_d.numel() < 2 or cand_off_d.numel() < 1 or offsets_d.numel() < 2
                or not span_text_d.numel() == span_start_d.numel() == span_len_d.numel() == span_first_d.numel() - 1):
            raise hipabi.KlError(_HYPOTHESIS_TENSORS % (
                "span_windows", "span_text int32 [S], span_start int64 [S], span_len int32 [S], span_first int64 [S + 1], "
                "pool int32 [n_pool], cand_off int64 [C + 1]"))
        S, C = int(span_text_d.numel()), int(cand_off_d.numel()) - 1
        row0, rows, left, ahead, max_len, T = int(row0), int(rows), int(left), int(ahead), int(max_len), int(T)
        if rows < 1 or T < 1 or not -2 ** 63 <= row0 < 2 ** 63:
            raise hipabi.KlError("span_windows: rows >= 1, T >= 1 (got %d, %d)" % (rows, T))
        return self._hypothesis_rows(
            self.lib.kl_span_windows, source, rows, T,
            (_ptr(span_text_d), _ptr(span_start_d), _ptr(span_len_d), _ptr(span_first_d), S,
             _ptr(pool_d) if pool_d.numel() else None, pool_d.numel(), _ptr(cand_off_d), C, row0, rows, left, ahead, max_len))

    def span_pick(self, cost_d, valid_d, span_first_d, min_gain, want_costs=True):
        """kl_span_pick: the choice among every span's candidates, on the device.  cost_d f64 [S + C] and valid_d int32 [S + C]
        per row of `span_windows`' numbering, span_first_d int64 [S + 1] -- DEVICE tensors.  Returns the DEVICE tensors (best
        int32 [S], gain f64 [S], cost with +inf where invalid f64 [S + C] -- None without want_costs): what
        `ratebulk.span_pick_host` states.  No synchronisation."""
        torch = self.torch
        tensors = (cost_d, valid_d, span_first_d)
        if (any(t is None for t in tensors) or [t.dtype for t in tensors] != [torch.float64, torch.int32, torch.int64]
                or any(t.dim() != 1 for t in tensors) or span_first_d.numel() < 2 or cost_d.numel() != valid_d.numel()
                or cost_d.numel() < span_first_d.numel() - 1 or not all(t.is_contiguous() and t.is_cuda for t in tensors)):
            raise hipabi.KlError("span_pick: cost f64 [S + C], valid int32 [S + C], span_first int64 [S + 1], contiguous, on the "
                                 "device")
        S = int(span_first_d.numel()) - 1
        C = int(cost_d.numel()) - S
        with self._launch():
            best = torch.empty(S, dtype=torch.int32, device=self.device)
            gain = torch.empty(S, dtype=torch.float64, device=self.device)
            out = torch.empty(S + C, dtype=torch.float64, device=self.device) if want_costs else None
            hipabi.check(self.lib.kl_span_pick(_ptr(cost_d), _ptr(valid_d), _ptr(span_first_d), S, C, float(min_gain), _ptr(best),
                                               _ptr(gain), _ptr(out), self._stream()), "kl_span_pick")
        return best, gain, out

    def rate_bits_take_all(self):
        """the accumulated bits of ALL streams as a DEVICE tensor (f64 [B]), the accumulators zeroed; no synchronisation"""
        with self._launch():
            out = self.rate_bits.clone()
            self.rate_bits.zero_()
        return out

    def rate_status_check(self):
        """raise if a scan hand-off timed out in a rate_window call since the last check (synchronises)"""
        if self._rate_status is not None and float(self._rate_status[3].item()) != 0.0:
            self._rate_status.zero_()        # one timed-out window must not fail every later call
            raise hipabi.KlError("persistent scan hand-off timed out (kl_rate_window)")

    def rate_bits_take(self, rows):
        """the accumulated bits of these streams as a DEVICE tensor (f64), the streams' accumulators zeroed; no synchronisation"""
        torch = self.torch
        with self._launch():
            r = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=self.device)
            out = self.rate_bits[r]
            self.rate_bits[r] = 0
        return out

    def rate_bits_read(self, reset=True):
        """bits [B] (numpy f64) accumulated per stream by rate_window since the last reset"""
        self.rate_status_check()
        if self.rate_bits is None:
            return np.zeros(0, dtype=np.float64)
        v = self.rate_bits.detach().cpu().numpy().copy()
        if reset:
            self.rate_bits.zero_()
        return v

    def draw_dropout_masks(self, B):
        """Inverted-dropout keep masks [L][B][W], time-constant per window (rating.py:146-152)."""
        keep = self._rng.random((self.depth, B, self.width)) >= DROPOUT_RATE
        m = (keep / (1.0 - DROPOUT_RATE)).astype(np.float32)
        m[0] = 1.0
        return m

    def draw_dropout_masks_device(self, B):
        """The same masks drawn in HBM (torch's generator, seeded from this engine's numpy generator on first use): at 3072
        streams the host drew 3.1 M random numbers per step, 6-8 ms beside 26 ms of GPU work."""
        torch = self.torch
        if getattr(self, "_tgen", None) is None:
            self._tgen = torch.Generator(device=self.device)
            self._tgen.manual_seed(int(self._rng.integers(0, 2 ** 31 - 1)))
        with torch.cuda.device(self.device):
            keep = torch.rand((self.depth, B, self.pwidth), device=self.device, generator=self._tgen) >= DROPOUT_RATE
            m = keep.to(torch.float32) / (1.0 - DROPOUT_RATE)
            m[0] = 1.0
        return m

    def assemble_windows(self, corpus, plan, T, n_ctx):
        """The batch of one step from the id corpus in HBM (streams.StreamBatcher): corpus int32 [n] and plan int64
        [B, 4 + n_ctx] (start, vlen, zero_col, zero_ctx, contexts) on the device -> (idx [B,T], ctx [B,T,n_ctx], tgt [B,T]),
        int32 device tensors, in one launch (kl_assemble_windows).  It runs on the engine stream: behind the plan's copy
        on the caller's stream, in front of the train_window / forward_window that consumes the batch."""
        torch = self.torch
        B = int(plan.shape[0])
        if (corpus.dtype != torch.int32 or plan.dtype != torch.int64 or plan.dim() != 2 or plan.shape[1] != 4 + n_ctx
                or not corpus.is_contiguous() or not plan.is_contiguous()
                or not corpus.is_cuda or not plan.is_cuda):
            raise hipabi.KlError("assemble_windows: corpus must be int32 [n], plan int64 [B, 4 + n_ctx], contiguous, on the device")
        with self._launch():
            idx = torch.empty((B, T), dtype=torch.int32, device=self.device)
            tgt = torch.empty((B, T), dtype=torch.int32, device=self.device)
            ctx = torch.empty((B, T, n_ctx), dtype=torch.int32, device=self.device)
            hipabi.check(self.lib.kl_assemble_windows(_ptr(corpus), corpus.numel(), _ptr(plan), B, int(T), int(n_ctx),
                                                      _ptr(idx), _ptr(ctx) if n_ctx else None, _ptr(tgt), self._stream()),
                         "kl_assemble_windows")
        return idx, ctx, tgt

    def ensure_training_buffers(self):
        torch = self.torch
        if self.grads is None:
            self.grads = torch.zeros_like(self.params)
            self.adam_m = torch.zeros_like(self.params)
            self.adam_v = torch.zeros_like(self.params)
            self.adam_t = 0

    def train_window(self, idx, ctx, tgt, masks=None):
        """forward + backward of one batch of B stateful windows; fills self.grads."""
        torch = self.torch
        self.ensure_training_buffers()
        if self.precision != hipabi.KL_PREC_BF16:
            self.prepare(hipabi.KL_PREC_BF16)
        with self._launch():
            idx_d = self._dev_i32(idx)
            B, T = idx_d.shape
            ctx_d = self._dev_i32(ctx) if self.n_ctx else None
            tgt_d = self._dev_i32(tgt)
            if self.states is None or self.states.shape[0] != B:
                self.reset_states(B)
            masks_d = None
            if masks is not None:
                masks_d = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(
                    np.ascontiguousarray(masks, dtype=np.float32)).to(self.device)
                if self.padded and masks_d.shape[-1] == self.width:      # (whatever the padded units get is multiplied by zero)
                    masks_d = torch.nn.functional.pad(masks_d, (0, self.pwidth - self.width), value=1.0).contiguous()
            parts = self._stream_groups(B, T)
            padded = [self._padded_streams(b1 - b0, T) for b0, b1 in parts]
            if len(parts) == 1 and padded[0] == B:
                ws = self._workspace(B, T, True)
                hipabi.check(self.lib.kl_train_window(self.handle, B, T, _ptr(idx_d), _ptr(ctx_d), _ptr(tgt_d),
                                                      _ptr(self.states), _ptr(masks_d), _ptr(self.grads),
                                                      _ptr(self.loss_acc), _ptr(ws), ws.numel(), self._stream()),
                             "kl_train_window")
                self._last_window = (B, T, 0, B, 1)
                return
            # More streams than one launch sequence addresses (the scans index a layer's gate rows, T * B * 4W bf16, with 32-bit
            # buffer offsets: 3072 streams at cfg2), or a count none of the fast kernels takes: the streams are independent, so
            # the batch runs as groups of streams one after the other -- each on the persistent-scan path, a group that is just
            # short of a fast count PADDED with dummy streams (targets -1: no loss, no gradient; kl_set_loss_rows keeps the
            # means those over the real streams) -- and the gradient of the mean over all B*T positions is the size-weighted sum
            # of the groups' gradients (the regularisers' part is the same in every group: the weights sum to 1).
            if self._part_grads is None:
                self._part_grads = torch.zeros_like(self.grads)
            if self._part_loss is None:
                self._part_loss = torch.zeros_like(self.loss_acc)
            ws = self._workspace(max(padded), T, True)
            for i, ((b0, b1), Bp) in enumerate(zip(parts, padded)):
                n = b1 - b0
                wgt = n / B
                self._part_loss.zero_()
                m = masks_d[:, b0:b1] if masks_d is not None else None
                # (-2, not the -1 of a padded tail: Keras counts an all-zero target row as a hit when class 0 wins, a dummy stream
                #  must not be counted at all)
                x, c, y, st = self._pad_group(b0, b1, Bp, idx_d, ctx_d, tgt_d, -2)
                if Bp != n:
                    if m is not None:
                        # (the dummy streams' keep-masks repeat real streams': the register-tile backward scan keeps a mask as
                        #  one bit per cell plus ONE scale per thread and refuses a mask with a second non-zero value)
                        # (_padded_streams adds at most as many dummy streams as there are real ones; a plan handed in may
                        #  add more, and a mask array short of Bp rows would be read beyond its end)
                        m = torch.cat([m, m[:, :Bp - n]], dim=1) if Bp - n <= n else m.repeat(1, -(-Bp // n), 1)[:, :Bp]
                    hipabi.check(self.lib.kl_set_loss_rows(self.handle, n), "kl_set_loss_rows")
                if m is not None:
                    m = m.contiguous()
                try:
                    hipabi.check(self.lib.kl_train_window(self.handle, Bp, T, _ptr(x), _ptr(c), _ptr(y), _ptr(st), _ptr(m),
                                                          _ptr(self._part_grads), _ptr(self._part_loss), _ptr(ws), ws.numel(),
                                                          self._stream()), "kl_train_window")
                finally:
                    if Bp != n:
                        hipabi.check(self.lib.kl_set_loss_rows(self.handle, 0), "kl_set_loss_rows")
                self._unpad_states(b0, b1, st)
                self._last_window = (Bp, T, b0, n, len(parts))
                if self.group_hook is not None:
                    self.group_hook(i, b0, b1, Bp)
                if i == 0:
                    torch.mul(self._part_grads, wgt, out=self.grads)
                    self.loss_acc[2] += self._part_loss[2]
                else:
                    self.grads.add_(self._part_grads, alpha=wgt)
                self.loss_acc[:2] += wgt * self._part_loss[:2]
                self.loss_acc[3] = torch.maximum(self.loss_acc[3], self._part_loss[3])

    def window_view(self):
        """Test hook (kl_test_window_view): where the last train_window left what its recurrence scans wrote.  Returns (view,
        workspace, info): the kl_window_view, the uint8 workspace tensor its byte offsets point into, and info = dict(B -- streams
        the kernels ran, dummy streams included --, T, first, n -- the real streams [first, first + n) of the batch that occupy
        rows [0, n) --, groups).  With several stream groups (groups > 1) the workspace holds the LAST group only.  Decoding:
        tests/window_ref.py.

        Every group of a grouped or padded window is reached through `group_hook` (default None: nothing is called, nothing
        else changes): when set, `train_window` and `forward_window` call group_hook(i, b0, b1, Bp) in their group loops --
        group i = streams [b0, b1) of the batch, run as Bp streams -- after the group's launch and `_unpad_states` and before
        its results are folded into `grads` / `loss_acc`.  There `_part_loss` (and, in `train_window`, `_part_grads`) are that
        group's own values, and in `train_window` this view describes group i.  The hook may synchronise; the engine does not
        on its behalf.  A batch that runs in one piece without padding calls no hook."""
        if self._last_window is None:
            raise hipabi.KlError("window_view: no training window has run")
        B, T, first, n, groups = self._last_window
        view = hipabi.KlWindowView()
        self.torch.cuda.synchronize(self.device)
        hipabi.check(self.lib.kl_test_window_view(self.handle, B, T, _ptr(self._ws), C.byref(view)), "kl_test_window_view")
        return view, self._ws, dict(B=B, T=T, first=first, n=n, groups=groups)

    def forward_view(self, B=None, T=None, ws=None):
        """Test hook (kl_test_forward_view): which scan family ran the last inference-layout window -- `forward_window` in split
        precision, `rate_window`, `rate_window_alts`; of a batch in several groups, the last group -- and where it left H, C, the
        (hi, lo) planes and P1.  Returns (view, workspace): the kl_forward_view and the uint8 tensor its byte offsets point into.
        B, T, ws: a window run through the library on a workspace of the caller's instead."""
        if ws is None:
            if self._last_forward is None:
                raise hipabi.KlError("forward_view: no inference window has run")
            B, T, ws = self._last_forward
        view = hipabi.KlForwardView()
        hipabi.check(self.lib.kl_test_forward_view(self.handle, int(B), int(T), _ptr(ws), C.byref(view)), "kl_test_forward_view")
        return view, ws

    def derived_view(self):
        """Test hook (kl_test_derived_view): where every operand array derived from the parameters lies and which groups of
        them match the parameters now.  Returns (view, derived): the kl_derived_view and the uint8 tensor its byte offsets
        point into, at the PADDED width.  Decoding and the arrays' definitions: tests/derived_ref.py."""
        view = hipabi.KlDerivedView()
        self.torch.cuda.synchronize(self.device)
        hipabi.check(self.lib.kl_test_derived_view(self.handle, C.byref(view)), "kl_test_derived_view")
        return view, self.derived

    def prepare_lazy(self, mask):
        """Test hook (kl_test_prepare_lazy): build the lazily built operand groups now (hipabi.KL_LAZY_* bits)."""
        with self._launch():
            hipabi.check(self.lib.kl_test_prepare_lazy(self.handle, int(mask), self._stream()), "kl_test_prepare_lazy")

    def _plan_512(self, B, limit):
        """[(streams, run as)] for a batch of B streams at width 512.  The second-generation scans take every multiple of 512
        from 1024 to 3072 streams (32 row groups x 2 .. 6 row blocks of 16, lstm_scan2.hip) and are faster per stream than the
        first generation at ANY count above 512 (tools/probe_shape_sweep.py, and timed against the alternatives by
        test_stream_plan_is_the_fastest): so a batch is rounded up to whole blocks of 512 streams with dummy streams, and what no
        single launch sequence addresses (`limit`: 32-bit offsets into a layer's gate rows, T * B * 4W bf16) or holds (3072) is
        cut into groups of the largest count (3584 -> 2560 + 1024, 4096 -> 3072 + 1024, 6144 -> 2 x 3072).  No table of measured
        times: nothing here has to be re-measured when a kernel changes."""
        if self.plan_override is not None:      # (tests time the rule's choice against other plans: [(streams, run as), ...])
            if sum(n for n, _run in self.plan_override) == B:
                return list(self.plan_override)
            return [(B, dict(self.plan_override).get(B, B))]
        unit = 512
        max_units = min(6, limit // unit)
        if not self.pad_streams or B <= unit or max_units < 2:
            if B <= limit:
                return [(B, B)]
            # (windows so long that fewer than 1024 streams fit a launch sequence: groups of the largest size the kernels address)
            chunk = limit // unit * unit if limit >= unit else max(16, limit // 16 * 16)
            return [(min(chunk, B - b0), min(chunk, B - b0)) for b0 in range(0, B, chunk)]
        # groups of the largest count first (the more row blocks a workgroup serves per step, the cheaper a stream: 3072 + 1024
        # beats 2 x 2048), the rest in one group -- or two, if it would otherwise be a single block of 512 (first generation)
        units = -(-B // unit)
        sizes = []
        while units > max_units + 1:
            sizes.append(max_units)
            units -= max_units
        if units > max_units:
            sizes += [max_units - 1, 2]
        elif units > 0:
            sizes.append(units)
        plan, left = [], B
        for u in sizes:
            run = u * unit
            n = min(run, left)
            plan.append((n, run))
            left -= n
        return [(n, run) for n, run in plan if n > 0]

    def _padded_streams(self, n, T):
        """the stream count a group of n streams is run at: width 512 see _plan_512; width 1024: the eight-wave scans give each of
        their 8 row groups whole blocks of 16 streams, a step costs ~6.3 ms per started 128 streams (300 streams 21.6 ms, 384: 19.2;
        1000: 59.6, 1024: 50.0) -- rounded up to a multiple of 128; else n"""
        if T < 3 or self.max_streams_per_launch:
            return n
        if self.pwidth == 1024:
            up = -(-n // 128) * 128
            return up if (self.pad_streams and n > 128 and up <= 0xfffffff0 // (T * 4 * self.pwidth * 2)) else n
        if self.pwidth != 512:
            return n
        plan = self._plan_512(n, 0xfffffff0 // (T * 4 * self.pwidth * 2))
        return plan[0][1] if len(plan) == 1 else n

    def _rating_groups(self, B):
        """[(first, end)] stream ranges of a rating window (split precision): the persistent split-precision scans keep a
        workgroup's weights in registers, one workgroup per CU, at most four 16-stream row blocks each -- 256 streams at depth 2 /
        width 512, 128 at depth 3 or 4, 512 at width 256 (lstm_scan.hip, kl_launch_scan_fwd_split) --; more streams in one call
        fell through to the launch-per-step kernels (1024 x 256 characters: 62.6 ms against 4 x 4.3).  Streams are independent:
        a larger batch runs as groups of that many."""
        W, L = self.pwidth, self.depth
        cus = min(256, self.torch.cuda.get_device_properties(self.device).multi_processor_count)
        if W in (64, 128, 256, 512) and L <= 4:
            cap = 64 * (cus // (L * (W // 16)))
        elif W == 1024:
            cap = 64 * (cus // (W // 16))
        else:
            cap = 0
        if cap <= 0 or B <= cap:
            return [(0, B)]
        return [(b0, min(B, b0 + cap)) for b0 in range(0, B, cap)]

    # Stream counts per (physical) width that run on the fastest kernels, and the count from which a batch that is none of them
    # is regrouped: width 512 -- what the second-generation scans take (32 row groups x 2..6 row blocks of 16, lstm_scan2.hip);
    # width 1024 -- the eight-wave scans serve up to 1024 streams (lstm_scan_w32.hip), beyond them the launch-per-step kernels
    # (2048 streams: 1.4 M chars/s against 5.2 M).  (Width 128 runs any count in one piece since round 4: lstm_scan_w128.hip.)
    FAST_STREAMS = {512: ((3072, 2048, 1536, 1024), 1025), 1024: ((1024, 512), 1025)}

    def _stream_groups(self, B, T):
        """[(first, end)] stream ranges of one training batch.  One range, unless (a) the batch is beyond what a launch
        sequence addresses (32-bit offsets into a layer's gate rows, T * B * 4W bf16) -- it would fall through to the
        launch-per-step kernels --, or (b) it is none of the stream counts the fastest kernels of its width take and large
        enough (FAST_STREAMS): then the largest such counts are peeled off as long as 512 streams or more remain
        (width 512: 2560 -> 2048 + 512, 3584 -> 3072 + 512, 4096 -> 3072 + 1024) and only the rest runs on the slower path."""
        limit = 0xfffffff0 // (T * 4 * self.pwidth * 2)
        if self.max_streams_per_launch:      # (never more than the offsets reach, whatever a caller asks for)
            limit = min(limit, self.max_streams_per_launch)
        if self.pwidth == 512 and T >= 3 and not self.max_streams_per_launch:
            parts, b0 = [], 0
            for n, _run in self._plan_512(B, limit):
                parts.append((b0, b0 + n))
                b0 += n
            return parts
        fast, regroup_from = self.FAST_STREAMS.get(self.pwidth, ((), 0))
        fast = [f for f in fast if f <= limit] if (T >= 3 and not self.max_streams_per_launch) else []
        parts, b0 = [], 0
        while B - b0 > 0:
            rem = B - b0
            take = rem
            if fast and rem not in fast and (rem >= regroup_from or b0 > 0 or rem > limit):
                f = next((f for f in fast if f <= rem and (rem - f == 0 or rem - f >= 512)), None)
                if f is not None:
                    take = f
            if take > limit:      # (no fast count applies: groups of the largest size the kernels address)
                take = limit // 512 * 512 if limit >= 512 else max(16, limit // 16 * 16)
            parts.append((b0, b0 + take))
            b0 += take
        return parts

    def adam_step(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, clip=1.0, grad_scale=1.0):
        """Keras-2.3 Adam(clipvalue=1.0) (rating.py:178).  grad_scale: the gradients are read as grads * grad_scale
        (1 / world size behind a summing all-reduce, distributed.GradSync.reduce)."""
        self.adam_t += 1
        with self._launch():
            hipabi.check(self.lib.kl_adam_step_scaled(self.handle, _ptr(self.grads), float(grad_scale), _ptr(self.adam_m),
                                                      _ptr(self.adam_v), self.adam_t, lr, b1, b2, eps, clip, self._stream()),
                         "kl_adam_step_scaled")

    def read_loss(self, reset=True):
        """(CE mean, accuracy, regulariser) accumulated since the last reset."""
        v = self.loss_acc.detach().cpu().numpy().copy()
        if reset:
            self.loss_acc.zero_()
        if v[3] != 0:
            raise hipabi.KlError("a persistent-scan hand-off timed out on the GPU (results of this window are invalid)")
        return float(v[0]), float(v[1]), float(v[2])

    # ------------------------------------------------------------------ incremental
    def ensure_pool(self, n_slots):
        torch = self.torch
        if self.pool is None or self.pool.shape[0] < n_slots:
            new = torch.zeros((n_slots, 2 * self.depth, self.pwidth), dtype=torch.float32, device=self.device)
            if self.pool is not None:
                new[:self.pool.shape[0]] = self.pool
            self.pool = new
        return self.pool

    def _i32(self, a):
        """device int32 view of `a` without a copy when it already is one"""
        torch = self.torch
        if isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.is_cuda and a.is_contiguous():
            return a
        return self._dev_i32(a)

    def step_slots(self, idx, ctx, slot_in, slot_out):
        """One LSTM step for n hypotheses whose states live in pool slots
        (device-resident variant of rating.py:578-639).  Returns probs tensor [n,V].

        A beam search calls this once per character, so the host side is kept short: the launches go
        onto the caller's current stream directly (every other engine call leaves that stream ordered
        after the engine stream, see _launch), nothing is copied when the arguments are device int32
        tensors, and the workspace size per n is cached."""
        torch = self.torch
        idx_d = self._i32(idx).reshape(-1)
        n = idx_d.numel()
        ctx_d = self._i32(ctx).reshape(n, -1) if self.n_ctx else None
        si = self._i32(slot_in).reshape(-1)
        so = self._i32(slot_out).reshape(-1)
        probs = torch.empty((n, self.voc_size), dtype=torch.float32, device=self.device)
        nws = self._step_ws_bytes.get(n)
        if nws is None:
            nws = self._step_ws_bytes[n] = int(self.lib.kl_step_workspace_bytes(self.handle, n))
        if self._step_ws is None or self._step_ws.numel() < nws:
            self._step_ws = torch.empty(nws, dtype=torch.uint8, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        hipabi.check(self.lib.kl_step_batch(self.handle, n, _ptr(idx_d), _ptr(ctx_d), _ptr(self.pool), _ptr(si),
                                            _ptr(so), _ptr(probs), _ptr(self._step_ws), self._step_ws.numel(),
                                            stream), "kl_step_batch")
        return probs

    def step_slots_heads(self, idx, ctx, slot_in, slot_out, k):
        """step_slots plus the first k state vectors of the new states, both on the HOST after ONE synchronising copy:
        (probs [n][V], heads [n][k][W]) as numpy arrays.  A beam search with history clustering (rating.py:887-916) needs
        both after every character; fetched one after the other they cost two round trips to an otherwise idle GPU."""
        torch = self.torch
        probs = self.step_slots(idx, ctx, slot_in, slot_out)
        so = self._i32(slot_out).reshape(-1)
        n = probs.shape[0]
        heads = self.pool.index_select(0, so.long())[:, :k, :self.width].reshape(n, -1)
        both = torch.cat([probs, heads], dim=1).cpu().numpy()
        return both[:, :self.voc_size], both[:, self.voc_size:].reshape(n, k, self.width)

    # ---- the step as a beam search issues it (kl_step_batch_host): host indices in, host results out, no stream synchronisation
    def _host_io(self, n, head_k):
        """page-locked, device-visible host buffers (kl_host_alloc) for up to n hypotheses: probabilities, head vectors,
        the arrival word; kept and grown as needed"""
        io = getattr(self, "_hio", None)
        if io is not None and io["n"] >= n and io["head_k"] >= head_k:
            return io
        if io is not None:
            self._host_io_free()
        n_cap = max(256, 1 << (n - 1).bit_length())
        sizes = {"probs": n_cap * self.voc_size * 4, "heads": max(1, n_cap * head_k * self.pwidth) * 4, "done": 64}
        io = {"n": n_cap, "head_k": head_k, "ticket": 0, "ptr": {}, "np": {}}
        for name, nbytes in sizes.items():
            ptr = self.lib.kl_host_alloc(nbytes)
            if not ptr:
                raise hipabi.KlError("kl_host_alloc(%d) failed" % nbytes)
            io["ptr"][name] = ptr
            ctype = C.c_uint32 if name == "done" else C.c_float
            io["np"][name] = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(nbytes // 4,))
        self._hio = io
        return io

    def _host_io_free(self):
        io = getattr(self, "_hio", None)
        if io is not None:
            self._hio = None
            self.torch.cuda.synchronize(self.device)      # (nothing may still be writing into the buffers)
            for ptr in io["ptr"].values():
                self.lib.kl_host_free(ptr)

    def step_host(self, idx, ctx, slot_in, slot_out, target=None, head_k=0, timeout=20.0):
        """One LSTM step for n hypotheses with HOST index arrays, results on the HOST (numpy): `Rater.predict`'s arithmetic
        (rating.py:578-639) at the latency a beam search sees.  Returns (probs, heads): probs [n][V], or [n] -- the
        probability of character target[i] for every row -- when `target` is given; heads [n][head_k][W] (the first head_k
        state vectors of the new states) or None.  The returned arrays are the caller's (copies of the delivery buffers)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        n = idx.shape[0]
        ctx = np.ascontiguousarray(ctx, dtype=np.int32).reshape(n, -1) if self.n_ctx else None
        si = np.ascontiguousarray(slot_in, dtype=np.int32).reshape(-1)
        so = np.ascontiguousarray(slot_out, dtype=np.int32).reshape(-1)
        tg = np.ascontiguousarray(target, dtype=np.int32).reshape(-1) if target is not None else None
        io = self._host_io(n, head_k)
        nws = self._step_ws_bytes.get(("host", n))
        if nws is None:
            nws = self._step_ws_bytes[("host", n)] = int(self.lib.kl_step_host_workspace_bytes(self.handle, n))
        if self._step_host_ws is None or self._step_host_ws.numel() < nws:
            self._step_host_ws = self.torch.empty(nws, dtype=self.torch.uint8, device=self.device)
        io["ticket"] = ticket = (io["ticket"] % 0x7fffffff) + 1
        stream = C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)
        hipabi.check(self.lib.kl_step_batch_host(
            self.handle, n, idx.ctypes.data, ctx.ctypes.data if ctx is not None else None, si.ctypes.data, so.ctypes.data,
            tg.ctypes.data if tg is not None else None, _ptr(self.pool), int(head_k), io["ptr"]["probs"], io["ptr"]["heads"],
            io["ptr"]["done"], ticket, _ptr(self._step_host_ws), self._step_host_ws.numel(), stream), "kl_step_batch_host")
        hipabi.check(self.lib.kl_step_wait(io["ptr"]["done"], ticket, float(timeout)), "kl_step_wait")
        probs = io["np"]["probs"][:n].copy() if tg is not None else io["np"]["probs"][:n * self.voc_size].reshape(n, -1).copy()
        heads = None
        if head_k:
            heads = io["np"]["heads"][:n * head_k * self.pwidth].reshape(n, head_k, self.pwidth)[:, :, :self.width].copy()
        return probs, heads

    # ---- a lattice edge in one call (kl_walk_batch_host): every row through all its characters, one wait
    def _walk_stage(self, nbytes):
        """the walk's own page-locked staging buffer (kl_host_alloc), kept and grown as needed"""
        st = getattr(self, "_wstage", None)
        if st is not None and st[1] >= nbytes:
            return st[0]
        if st is not None:
            self.torch.cuda.synchronize(self.device)      # (nothing may still be reading it)
            self.lib.kl_host_free(st[0])
            self._wstage = None
        cap = max(1 << 16, 1 << (int(nbytes) - 1).bit_length())
        ptr = self.lib.kl_host_alloc(cap)
        if not ptr:
            raise hipabi.KlError("kl_host_alloc(%d) failed" % cap)
        self._wstage = (ptr, cap)
        return ptr

    def walk_host(self, lens, idx, target, ctx, slot_in, slot_step, head_k=0, timeout=20.0, wait=True):
        """len(lens) rows walked through lens[i] chained LSTM steps each, HOST index arrays in, results on the HOST:
        idx / target / slot_step are ragged (row i at the prefix sum of lens), ctx [n][n_ctx], slot_in [n].  Step t of a row
        reads the state step t - 1 left (slot_in[i] for the first) and leaves its own in slot_step[off + t]; returns
        (tprob, heads): tprob ragged float32, the probability of target[off + t] after step t; heads [n][head_k][W] (the
        first head_k state vectors of every row's FINAL state) or None.  One engine call and one wait, whatever the lengths."""
        lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        n = lens.shape[0]
        total = int(lens.sum())
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        tg = np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
        so = np.ascontiguousarray(slot_step, dtype=np.int32).reshape(-1)
        si = np.ascontiguousarray(slot_in, dtype=np.int32).reshape(-1)
        ctx = np.ascontiguousarray(ctx, dtype=np.int32).reshape(n, -1) if self.n_ctx else None
        if n < 1 or idx.shape[0] != total or tg.shape[0] != total or so.shape[0] != total or si.shape[0] != n:
            raise hipabi.KlError("walk_host: %d rows of %d steps in all do not match the index arrays" % (n, total))
        # (_host_io's probability buffer holds n_cap * V floats: `rows` such that it takes one float per step)
        io = self._host_io(max(n, -(-total // self.voc_size)), head_k)
        key = ("walk", n, total)
        sizes = self._step_ws_bytes.get(key)
        if sizes is None:
            if len(self._step_ws_bytes) > 4096:      # (edges come in many shapes: do not keep them all for ever)
                self._step_ws_bytes.clear()
            sizes = self._step_ws_bytes[key] = (int(self.lib.kl_walk_workspace_bytes(self.handle, n, total)),
                                                int(self.lib.kl_walk_stage_bytes(self.handle, n, total)))
        nws, nstage = sizes
        if self._walk_ws is None or self._walk_ws.numel() < nws:
            self._walk_ws = self.torch.empty(max(nws, 1 << 20), dtype=self.torch.uint8, device=self.device)
        stage = self._walk_stage(nstage)
        io["ticket"] = ticket = (io["ticket"] % 0x7fffffff) + 1
        stream = C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)
        hipabi.check(self.lib.kl_walk_batch_host(
            self.handle, n, lens.ctypes.data, idx.ctypes.data, tg.ctypes.data, ctx.ctypes.data if ctx is not None else None,
            si.ctypes.data, so.ctypes.data, _ptr(self.pool), int(head_k), io["ptr"]["probs"], io["ptr"]["heads"], stage,
            io["ptr"]["done"], ticket, _ptr(self._walk_ws), self._walk_ws.numel(), stream), "kl_walk_batch_host")
        if not wait:      # (edge_round: the caller enqueues more behind the walk and waits once, with `walk_wait`)
            return io, ticket, total
        hipabi.check(self.lib.kl_step_wait(io["ptr"]["done"], ticket, float(timeout)), "kl_step_wait")
        tprob = io["np"]["probs"][:total].copy()
        heads = None
        if head_k:
            heads = io["np"]["heads"][:n * head_k * self.pwidth].reshape(n, head_k, self.pwidth)[:, :, :self.width].copy()
        return tprob, heads

    # ---- the beam bookkeeping of many lattice edges (kl_edge_costs, kl_edge_decode): one round of Rater.rate_best_batch
    def edge_round(self, arrays, lm_weight, batch_size, beam_width, depth_k=0, dist=0.0, timeout=20.0):
        """One round of `lattice_batch.decode_lattices` on the device: uploads the edges' arrays (EdgeBatch.arrays()) in ONE
        transfer and returns an EdgeRound -- `walk(args, pair_off, n_pairs)` per walk call of the round, then `finish()`."""
        return EdgeRound(self, arrays, lm_weight, batch_size, beam_width, depth_k, dist, timeout)

    # ---- generate's beam search on the device (kl_beam_expand): expansion and pruning where the probabilities already are
    def beam_expand(self, probs, cum_in, slot_new, zero_slot, fan, floor, valid=None, out=None):
        """One expansion and pruning step of generate's search (rating.py:689-707) for the rows of `probs` (device [rows][V]
        f32, what step_slots returned): cum_in [rows] f32 (+inf: dead row), slot_new [rows] int32 (the slots that step
        wrote), valid [V] uint8 or None (every id except 0) -- device tensors.  Returns device tensors (idx [rows],
        slot_in_next [rows], cum_next [rows], parent [rows], n_live [1]); `out` = those five, preallocated.  Launches on the
        caller's current stream, no synchronisation (the order: genbeam.py, include/keraslm_hip.h)."""
        torch = self.torch
        rows = int(probs.shape[0])
        fan = int(fan)
        if (probs.dtype != torch.float32 or not probs.is_contiguous() or probs.shape[1] != self.voc_size
                or cum_in.dtype != torch.float32 or cum_in.numel() != rows or slot_new.dtype != torch.int32
                or slot_new.numel() != rows or (valid is not None and (valid.dtype != torch.uint8 or valid.numel() != self.voc_size))):
            raise hipabi.KlError("beam_expand: probs f32 [rows][V], cum_in f32 [rows], slot_new int32 [rows], valid uint8 [V]")
        if out is None:
            out = (torch.empty(rows, dtype=torch.int32, device=self.device), torch.empty(rows, dtype=torch.int32, device=self.device),
                   torch.empty(rows, dtype=torch.float32, device=self.device), torch.empty(rows, dtype=torch.int32, device=self.device),
                   torch.empty(1, dtype=torch.int32, device=self.device))
        idx, slot_in, cum, parent, n_live = out
        key = ("beam", rows, fan)
        nws = self._step_ws_bytes.get(key)
        if nws is None:
            nws = self._step_ws_bytes[key] = int(self.lib.kl_beam_workspace_bytes(self.handle, rows, fan))
        if self._beam_ws is None or self._beam_ws.numel() < nws:
            self._beam_ws = torch.empty(max(nws, 1 << 16), dtype=torch.uint8, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        # (the log's row doubles as the next step's input: the *_log and *_next pointers are the same)
        hipabi.check(self.lib.kl_beam_expand(self.handle, rows, fan, float(floor), _ptr(probs), _ptr(valid), _ptr(cum_in),
                                             _ptr(slot_new), int(zero_slot), _ptr(idx), _ptr(slot_in), _ptr(cum), _ptr(parent),
                                             _ptr(idx), _ptr(cum), _ptr(n_live), _ptr(self._beam_ws), self._beam_ws.numel(),
                                             stream), "kl_beam_expand")
        return out

    def beam_generate(self, idx0, slot0, ctx, length, rows, fan, floor, valid, slots_a, slots_b, zero_slot):
        """The whole search of `Rater.generate` enqueued back to back: for step s, step_slots on `rows` rows (dead rows run
        too: they read zero_slot and write their own slot) into slot set s & 1 (reading the other), then beam_expand.  The
        first step has one live row (character idx0 in the state of slot0).  No host synchronisation inside the loop; at the
        end ONE copy brings the log.  Returns (parent [length][rows] int32, idx [length][rows] int32, cum [length][rows]
        float32, n_live [length] int32) as numpy arrays (genbeam.backtrack reads them).  The pool must hold all slots named."""
        torch = self.torch
        length, rows = int(length), int(rows)
        n = length * rows
        sets = (np.asarray(slots_a, dtype=np.int32).reshape(-1), np.asarray(slots_b, dtype=np.int32).reshape(-1))
        if len(sets[0]) != rows or len(sets[1]) != rows or rows < 1 or length < 1:
            raise hipabi.KlError("beam_generate: two sets of %d slots and a positive length, please" % rows)
        n_ctx = self.n_ctx
        # everything the loop reads from the host in ONE upload: slot sets, context rows, the first fringe (cum as its bits)
        first = np.zeros((3, rows), dtype=np.int32)
        first[0, 0], first[1, :], first[1, 0] = idx0, zero_slot, slot0
        first[2, :] = np.array([np.inf], dtype=np.float32).view(np.int32)[0]
        first[2, 0] = 0
        head = np.concatenate([sets[0], sets[1], first.reshape(-1),
                               np.tile(np.asarray(ctx, dtype=np.int32).reshape(1, -1), (rows, 1)).reshape(-1)])
        with torch.cuda.device(self.device):
            head_d = self.to_device_i32(head)
            valid_d = None
            if valid is not None:
                valid_d = torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)).to(self.device, non_blocking=True)
            set_d = (head_d[:rows], head_d[rows:2 * rows])
            idx, slot_in, cum = head_d[2 * rows:3 * rows], head_d[3 * rows:4 * rows], head_d[4 * rows:5 * rows].view(torch.float32)
            ctx_d = head_d[5 * rows:].view(rows, n_ctx) if n_ctx else None
            log = torch.empty(3 * n + length, dtype=torch.int32, device=self.device)      # parent, idx, cum (bits), live counts
            parent_rows = log[:n].view(length, rows).unbind(0)
            idx_rows = log[n:2 * n].view(length, rows).unbind(0)
            cum_rows = log[2 * n:3 * n].view(torch.float32).view(length, rows).unbind(0)
            live = log[3 * n:]
            slot_next = (torch.empty(rows, dtype=torch.int32, device=self.device),
                         torch.empty(rows, dtype=torch.int32, device=self.device))
            for s in range(length):
                new = set_d[s & 1]
                probs = self.step_slots(idx, ctx_d, slot_in, new)
                self.beam_expand(probs, cum, new, zero_slot, fan, floor, valid_d,
                                 out=(idx_rows[s], slot_next[s & 1], cum_rows[s], parent_rows[s], live[s:s + 1]))
                idx, slot_in, cum = idx_rows[s], slot_next[s & 1], cum_rows[s]
            host = log.cpu().numpy()      # (the one wait of the search)
        return (host[:n].reshape(length, rows), host[n:2 * n].reshape(length, rows),
                host[2 * n:3 * n].view(np.float32).reshape(length, rows), host[3 * n:])

    # ---- sampling on the device (kl_sample_pick): one drawn character per chain where the probabilities already are
    def sample_pick(self, probs, cum_in, temperature, top_k, floor, seed, step, valid=None, out=None, row0=0):
        """One drawn character for every row of `probs` (device [rows][V] f32, what step_slots returned): cum_in [rows] f32,
        valid [V] uint8 or None (every id except 0) -- device tensors.  Row r draws with the uniform number of (seed, step,
        row0 + r) (gensample.philox_uniform).  Returns device tensors (idx [rows] int32, cum_next [rows] f32, u [rows] f32);
        `out` = those three, preallocated (cum_next may be cum_in).  Launches on the caller's current stream, no
        synchronisation (the contract: include/keraslm_hip.h, gensample.py)."""
        torch = self.torch
        rows = int(probs.shape[0])
        if (probs.dtype != torch.float32 or not probs.is_contiguous() or probs.shape[1] != self.voc_size
                or cum_in.dtype != torch.float32 or cum_in.numel() != rows
                or (valid is not None and (valid.dtype != torch.uint8 or valid.numel() != self.voc_size))):
            raise hipabi.KlError("sample_pick: probs f32 [rows][V], cum_in f32 [rows], valid uint8 [V]")
        if out is None:
            out = (torch.empty(rows, dtype=torch.int32, device=self.device), torch.empty(rows, dtype=torch.float32, device=self.device),
                   torch.empty(rows, dtype=torch.float32, device=self.device))
        idx, cum, u = out
        key = ("sample", rows)
        nws = self._step_ws_bytes.get(key)
        if nws is None:
            nws = self._step_ws_bytes[key] = int(self.lib.kl_sample_workspace_bytes(self.handle, rows))
        if self._sample_ws is None or self._sample_ws.numel() < nws:
            self._sample_ws = torch.empty(max(nws, 1 << 16), dtype=torch.uint8, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        hipabi.check(self.lib.kl_sample_pick_from(self.handle, rows, int(row0) & 0xffffffff, _ptr(probs), _ptr(valid),
                                                  float(temperature), int(top_k), float(floor), int(seed) & 0xffffffffffffffff,
                                                  int(step) & 0xffffffff, _ptr(cum_in), _ptr(idx), _ptr(cum), _ptr(u),
                                                  _ptr(self._sample_ws), self._sample_ws.numel(), stream), "kl_sample_pick")
        return out

    def sample_generate(self, idx0, slot0, ctx, length, rows, temperature, top_k, floor, seed, valid, slots_a, slots_b, zero_slot,
                        keep_probs=False, row0=0):
        """`rows` chains of `Rater.sample` enqueued back to back: for step s, step_slots into slot set s & 1, then sample_pick
        with step = s.  Row r always continues its own chain -- its next slot_in is the slot it just wrote --; at step 0 every
        row reads slot0 and feeds idx0.  No host synchronisation inside the loop; at the end ONE copy brings the log.
        Returns (idx [length][rows] int32, cum [length][rows] float32, u [length][rows] float32) as numpy arrays
        (gensample.spell reads them); keep_probs: also every step's probabilities [length][rows][V] (for tests).  The pool
        must hold all slots named; zero_slot is not used (the signature is beam_generate's)."""
        torch = self.torch
        length, rows = int(length), int(rows)
        n = length * rows
        sets = (np.asarray(slots_a, dtype=np.int32).reshape(-1), np.asarray(slots_b, dtype=np.int32).reshape(-1))
        if len(sets[0]) != rows or len(sets[1]) != rows or rows < 1 or length < 1:
            raise hipabi.KlError("sample_generate: two sets of %d slots and a positive length, please" % rows)
        n_ctx = self.n_ctx
        # everything the loop reads from the host in ONE upload: slot sets, the first step's inputs (cum 0.0 = zero bits), context rows
        first = np.zeros((3, rows), dtype=np.int32)
        first[0, :], first[1, :] = idx0, slot0
        head = np.concatenate([sets[0], sets[1], first.reshape(-1),
                               np.tile(np.asarray(ctx, dtype=np.int32).reshape(1, -1), (rows, 1)).reshape(-1)])
        with torch.cuda.device(self.device):
            head_d = self.to_device_i32(head)
            valid_d = None
            if valid is not None:
                valid_d = torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)).to(self.device, non_blocking=True)
            set_d = (head_d[:rows], head_d[rows:2 * rows])
            idx, slot_in, cum = head_d[2 * rows:3 * rows], head_d[3 * rows:4 * rows], head_d[4 * rows:5 * rows].view(torch.float32)
            ctx_d = head_d[5 * rows:].view(rows, n_ctx) if n_ctx else None
            log = torch.empty(3 * n, dtype=torch.int32, device=self.device)      # idx, cum (bits), u (bits)
            idx_rows = log[:n].view(length, rows).unbind(0)
            cum_rows = log[n:2 * n].view(torch.float32).view(length, rows).unbind(0)
            u_rows = log[2 * n:].view(torch.float32).view(length, rows).unbind(0)
            kept = []
            for s in range(length):
                new = set_d[s & 1]
                probs = self.step_slots(idx, ctx_d, slot_in, new)
                self.sample_pick(probs, cum, temperature, top_k, floor, seed, s, valid_d,
                                 out=(idx_rows[s], cum_rows[s], u_rows[s]), row0=row0)
                idx, slot_in, cum = idx_rows[s], new, cum_rows[s]
                if keep_probs:
                    kept.append(probs)
            host = log.cpu().numpy()      # (the one wait of the call)
            out = (host[:n].reshape(length, rows), host[n:2 * n].view(np.float32).reshape(length, rows),
                   host[2 * n:].view(np.float32).reshape(length, rows))
            if keep_probs:
                out += (torch.stack(kept).cpu().numpy(),)
        return out

    def to_device_i32(self, a):
        """one host-to-device transfer of an int32 array (rows stay contiguous views)"""
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device, non_blocking=True)

    def pool_heads(self, slots, k):
        """first k state vectors of the given slots, [n][k][W] on the host"""
        idx = self.torch.as_tensor(np.asarray(slots), device=self.device, dtype=self.torch.long)
        return self.pool[idx, :k, :self.width].cpu().numpy()

    def state_dist2(self, a, b, k):
        torch = self.torch
        a_d, b_d = self._dev_i32(a).reshape(-1), self._dev_i32(b).reshape(-1)
        out = torch.empty(a_d.numel(), dtype=torch.float32, device=self.device)
        with self._launch():
            hipabi.check(self.lib.kl_state_dist2(self.handle, a_d.numel(), _ptr(self.pool), _ptr(a_d), _ptr(b_d), int(k),
                                                 _ptr(out), self._stream()), "kl_state_dist2")
        return out

    # ------------------------------------------------------------------ pool access (host <-> HBM)
    def pool_zero(self, slots):
        with self._launch():
            self.pool[self.torch.as_tensor(list(slots), device=self.device, dtype=self.torch.long)] = 0

    def pool_read(self, slots):
        """states of the given slots as a numpy array [n][2L][W]"""
        with self._launch():
            out = self.pool[self.torch.as_tensor(list(slots), device=self.device, dtype=self.torch.long)][:, :, :self.width]
        return out.cpu().numpy()

    def pool_write(self, slots, values):
        with self._launch():
            v = self.torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(self.device)
            if self.padded and v.shape[-1] == self.width:
                v = self.torch.nn.functional.pad(v, (0, self.pwidth - self.width))
            self.pool[self.torch.as_tensor(list(slots), device=self.device, dtype=self.torch.long)] = v



class EdgeRound(object):
    """The device side of one round of many lattices' decoding (lib/lattice_batch.py): the walk's probabilities become costs
    (kl_edge_costs, reading the walk's host-visible result buffer on the walk's stream -- the host does not wait in between),
    kl_edge_decode takes every edge's bookkeeping, ONE copy brings the outputs and the host waits ONCE, for at most
    `timeout` seconds.  A round whose walk goes in several calls waits for each call but the last before it issues the next
    (the staging buffers belong to a call until it has arrived).
    For tests: `costs_from(probs)` computes the costs from given f32 probabilities instead of a walk, `set_costs(cost)`
    uploads given f64 costs; `finish(want_costs=True)` also returns the device's cost array."""
    F64 = ("cum_in", "alt_conf", "pre_cost")
    I32 = ("desc", "slot_in", "alt_len", "alt_class", "step_off", "final_slot", "pre_class", "pre_slot", "pair_alt")

    def __init__(self, lm, arrays, lm_weight, batch_size, beam_width, depth_k, dist, timeout):
        torch = lm.torch
        self.lm, self.timeout = lm, float(timeout)
        self.lm_weight, self.batch_size, self.beam_width = float(lm_weight), int(batch_size), int(beam_width)
        self.depth_k, self.dist = int(depth_k), float(dist)
        desc = arrays["desc"]
        self.n_edges = int(desc.shape[0])
        self.n_tracks = int(arrays["step_off"].shape[0])
        self.n_pairs = int(arrays["pair_alt"].shape[0])
        tracks = desc[:, 0].astype(np.int64) * desc[:, 1]
        fits = tracks[tracks <= 1024]
        self.cap = int(fits.max()) if len(fits) else 1      # (an edge above the limit gets its status from the kernel)
        # ---- one upload: the f64 arrays, then the int32 arrays, every part 8-byte aligned
        parts, self.off, at = [], {}, 0
        for name in self.F64 + self.I32:
            a = np.ascontiguousarray(arrays[name], dtype=np.float64 if name in self.F64 else np.int32).reshape(-1)
            raw = a.view(np.uint8)
            pad = (-len(raw)) % 8
            self.off[name] = at
            parts.append(raw)
            if pad:
                parts.append(np.zeros(pad, dtype=np.uint8))
            at += len(raw) + pad
        host = np.concatenate(parts) if at else np.zeros(8, dtype=np.uint8)
        self.stream = torch.cuda.current_stream(lm.device)
        with torch.cuda.device(lm.device):
            self.inp = torch.from_numpy(host).to(lm.device, non_blocking=True)
            self.cost = torch.empty(max(1, self.n_pairs), dtype=torch.float64, device=lm.device)
            self.out_bytes = int(lm.lib.kl_edge_decode_out_bytes(self.n_edges, self.beam_width, self.n_tracks, self.n_pairs))
            if not self.out_bytes:
                raise hipabi.KlError("edge_round: %d edges, %d tracks, %d pairs" % (self.n_edges, self.n_tracks, self.n_pairs))
            self.out = torch.empty(self.out_bytes, dtype=torch.uint8, device=lm.device)
        self.pending = None      # (io, ticket, pair_off, n_pairs) of the walk call that has not arrived yet
        self.tprob = np.zeros(self.n_pairs, dtype=np.float32)
        self.keep = []

    def _in(self, name):
        return self.inp.data_ptr() + self.off[name]

    def _stream(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _arrived(self):
        if self.pending is not None:
            io, ticket, p0, n = self.pending
            hipabi.check(self.lm.lib.kl_step_wait(io["ptr"]["done"], ticket, self.timeout), "kl_step_wait")
            self.tprob[p0:p0 + n] = io["np"]["probs"][:n]
            self.pending = None

    def walk(self, args, pair_off, n_pairs):
        """one walk call (walk_host's arguments) whose rows are the pairs pair_off .. pair_off + n_pairs - 1 of the round"""
        self._arrived()
        io, ticket, total = self.lm.walk_host(*args, wait=False)
        if total != n_pairs:
            raise hipabi.KlError("edge_round: a walk of %d pairs where %d were announced" % (total, n_pairs))
        hipabi.check(self.lm.lib.kl_edge_costs(n_pairs, io["ptr"]["probs"], self._in("pair_alt") + 4 * pair_off, self._in("alt_conf"),
                                               self.lm_weight, self.cost.data_ptr() + 8 * pair_off, self._stream()), "kl_edge_costs")
        self.pending = (io, ticket, pair_off, n_pairs)

    def costs_from(self, probs):
        probs = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1)
        assert len(probs) == self.n_pairs
        with self.lm.torch.cuda.device(self.lm.device):
            dev = self.lm.torch.from_numpy(probs).to(self.lm.device)
        self.keep.append(dev)
        hipabi.check(self.lm.lib.kl_edge_costs(self.n_pairs, dev.data_ptr(), self._in("pair_alt"), self._in("alt_conf"), self.lm_weight,
                                               self.cost.data_ptr(), self._stream()), "kl_edge_costs")

    def set_costs(self, cost):
        cost = np.ascontiguousarray(cost, dtype=np.float64).reshape(-1)
        assert len(cost) == self.n_pairs
        self.cost[:self.n_pairs].copy_(self.lm.torch.from_numpy(cost))

    def decode_args(self):
        """the arguments of kl_edge_decode as this round passes them (tests vary them)"""
        lm = self.lm
        return [lm.handle, self.n_edges] + [self._in(k) for k in ("desc", "cum_in", "alt_len", "alt_class", "step_off",
                                                                   "final_slot", "pre_cost", "pre_class", "pre_slot")] + [
            self.cost.data_ptr(), _ptr(lm.pool) if self.depth_k else None, self.depth_k, self.dist, self.batch_size, self.beam_width,
            self.cap, self.n_tracks, self.n_pairs, self.out.data_ptr(), self.out_bytes, self._stream()]

    def finish(self, want_costs=False):
        """the decode launch, the one copy and the one wait; {count, status, ref, cost, consumed, when, tprob}"""
        lm, torch = self.lm, self.lm.torch
        hipabi.check(lm.lib.kl_edge_decode(*self.decode_args()), "kl_edge_decode")
        with torch.cuda.device(lm.device):
            host = torch.empty(self.out_bytes, dtype=torch.uint8, pin_memory=True)
            host.copy_(self.out, non_blocking=True)
            cost_host = None
            if want_costs:
                cost_host = torch.empty(self.n_pairs, dtype=torch.float64, pin_memory=True)
                cost_host.copy_(self.cost[:self.n_pairs], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        t0 = time.monotonic()
        while not done.query():
            if time.monotonic() - t0 > self.timeout:
                raise hipabi.KlError("edge_round: no result after %.0f s" % self.timeout)
        self._arrived()      # (behind the event on the same stream: it has arrived)
        raw = host.numpy()
        e, bw = self.n_edges, self.beam_width
        up8 = lambda n: (n + 7) & ~7
        at = 0
        out = {"cost": raw[at:at + e * bw * 8].view(np.float64).reshape(e, bw)}
        at += e * bw * 8
        for name, n in (("count", e), ("status", e), ("ref", e * bw), ("consumed", self.n_tracks), ("when", self.n_pairs)):
            out[name] = raw[at:at + 4 * n].view(np.int32)
            at += up8(4 * n)
        out["ref"] = out["ref"].reshape(e, bw)
        out["tprob"] = self.tprob
        if want_costs:
            out["step_cost"] = cost_host.numpy()
        return out
