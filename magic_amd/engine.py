"""Engine: one libmvae context on one GPU, with torch views of its device memory.

PyTorch is plumbing here (device memory, streams, RNG for inputs, torch.distributed);
every arithmetic step of the training path runs in the HIP kernels of ``libmvae.so``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .config import MVAEConfig
from .overlap_input import PairBatch

PARAM_ORDER_DEAD = ("dec_out_log_sigma_W", "dec_out_log_sigma_b")


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("expected a contiguous float32 device tensor")
    return t.data_ptr()


def _iptr(t: torch.Tensor):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError("expected a contiguous int32 device tensor")
    return t.data_ptr()


class Engine:
    """Owns an ``mvae_ctx``. Tensors passed in must be contiguous float32 on ``device``; wherever
    a method takes the batch ``x`` it also takes an ``overlap_input.PairBatch``."""

    def __init__(self, cfg: MVAEConfig, device: int = 0):
        if not torch.cuda.is_available():
            raise _lib.MVAELibraryError("no GPU visible: libmvae runs on MI355X (gfx950) only")
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = device
        self.dev = torch.device("cuda", device)
        c = _lib.mvae_cfg()
        c.image_size = cfg.image_size
        c.batch = cfg.batch
        c.global_batch = cfg.gbatch
        c.n_enc = len(cfg.enc)
        if not 1 <= c.n_enc <= _lib.MVAE_MAX_ENC:
            raise ValueError("encoder depth out of range")
        for i, e in enumerate(cfg.enc):
            c.enc[i] = e
        c.dec[0], c.dec[1] = cfg.dec
        c.latent = cfg.latent
        c.act = _lib.ACT[cfg.act]
        c.metric = _lib.METRIC[cfg.metric]
        c.reciprocal = int(cfg.reciprocal)
        c.deform_weight = cfg.deform_weight
        c.lr[0], c.lr[1] = cfg.lr
        c.beta1, c.beta2, c.epsilon = cfg.beta1, cfg.beta2, cfg.epsilon
        c.precision = _lib.PREC[cfg.precision]
        c.seed = cfg.seed
        c.conv = int(getattr(cfg, "conv", False))
        torch.cuda.set_device(device)
        torch.cuda.init()
        h = C.c_void_p()
        opts = getattr(cfg, "options", "") or None
        rc = self.lib.mvae_create_ex(C.byref(c), device, opts.encode() if opts else None, C.byref(h))
        if rc != 0:
            raise _lib.MVAEError(rc, (self.lib.mvae_last_error(None) or b"").decode())
        self.ctx = h.value
        self._keep = []
        self._views: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self.losses = self.buffer(_lib.BUF_LOSSES)
        self.grads = self.buffer(_lib.BUF_GRADS)
        self.colsq = self.buffer(_lib.BUF_COLSQ)
        self.coldot = self.buffer(_lib.BUF_COLDOT)
        self.dist = self.buffer(_lib.BUF_DIST)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "ctx", None):
            torch.cuda.synchronize(self.dev)
            self._views.clear()
            self.losses = self.grads = self.colsq = self.coldot = self.dist = None
            self.lib.mvae_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        return _lib.check(self.lib, self.ctx, rc)

    @property
    def stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    # ------------------------------------------------------------------ memory views
    def buffer(self, which: int) -> torch.Tensor:
        p = C.c_void_p()
        n = C.c_size_t()
        self._check(self.lib.mvae_buffer(self.ctx, which, C.byref(p), C.byref(n)))
        return _lib.device_view(p.value, (n.value,), (1,), self.device, self._keep)

    def tensors(self, kind: int = _lib.KIND_PARAM) -> Dict[str, torch.Tensor]:
        """Name -> view, in the reference's variable creation order (``11a/vae.py:85-153``).
        Weights are [fan_in, fan_out] (y = x W), biases [fan_out]."""
        key = (kind,)
        if key in self._views:
            return self._views[key]
        out = {}
        n = self.lib.mvae_param_count(self.ctx)
        t = _lib.mvae_tensor()
        for i in range(n):
            rc = self.lib.mvae_param_info(self.ctx, kind, i, C.byref(t))
            if rc != 0:
                continue  # e.g. decoder variables have no metric-optimizer state
            name = t.name.decode()
            if t.rows == 1 and not name.endswith("_W"):
                v = _lib.device_view(t.data, (t.cols,), (1,), self.device, self._keep)
            else:
                v = _lib.device_view(t.data, (t.rows, t.cols), (t.ld, 1), self.device, self._keep)
            out[name] = v
        self._views[key] = out
        return out

    def params(self) -> Dict[str, torch.Tensor]:
        return self.tensors(_lib.KIND_PARAM)

    def sync_params(self):
        """Refresh the bf16 plane images of the parameters after writing the fp32 masters
        through the views (bf16 / f32x modes; a no-op in fp32 mode)."""
        self._check(self.lib.mvae_sync_params(self.ctx, self.stream))

    def load_params(self, P: Dict[str, np.ndarray]):
        views = self.params()
        for k, v in P.items():
            views[k].copy_(torch.as_tensor(np.asarray(v, np.float32)).to(self.dev))
        self.sync_params()
        torch.cuda.synchronize(self.dev)

    def init_params(self, seed: int = 0):
        """Xavier-uniform weights (``11a/utils.py:484-491``), zero biases (``11a/vae.py:116-153``),
        drawn on the host from a seeded generator in the reference's creation order."""
        rng = np.random.default_rng(seed)
        views = self.params()
        for name, v in views.items():
            if v.dim() == 2:
                fan_in, fan_out = v.shape
                if name.startswith("enc_conv"):  # slim xavier: receptive field on both fans
                    fan_out *= 25
                hi = np.sqrt(6.0 / (fan_in + fan_out))
                v.copy_(torch.from_numpy(rng.uniform(-hi, hi, size=tuple(v.shape)).astype(np.float32)).to(self.dev))
            else:
                v.zero_()
        self.sync_params()
        torch.cuda.synchronize(self.dev)

    def get_step(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.mvae_get_step(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_step(self, t1: int, t2: int):
        self._check(self.lib.mvae_set_step(self.ctx, t1, t2))

    def set_shard(self, row_offset: int):
        """This rank's first row in the global batch (the internal eps sampler draws the
        rank's slice of the global stream)."""
        self._check(self.lib.mvae_set_shard(self.ctx, row_offset))

    def get_rng(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mvae_get_rng(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_rng(self, train: int, eval_: int):
        self._check(self.lib.mvae_set_rng(self.ctx, train, eval_))

    # ------------------------------------------------------------------ step phases
    def _xin(self, x):
        if tuple(x.shape) != (self.cfg.batch, 3 * self.cfg.D):
            raise ValueError(f"X must be [{self.cfg.batch}, {3 * self.cfg.D}] (got {tuple(x.shape)})")
        if isinstance(x, PairBatch):
            return self._pairs(x)
        return _ptr(x)

    def _pairs(self, pb: PairBatch):
        """The ``mvae_pairs`` descriptor of a ``PairBatch`` (tensors re-checked: they are mutable
        attributes), or ``mvae_xpairs`` when it carries a ``key_idx``: the key table then only has to
        share H and W with the lock table. Square tables only, as ``cfg.image_size``."""
        kidx = getattr(pb, "key_idx", None)
        for t, dt in ((pb.locks, torch.uint8), (pb.keys, torch.uint8), (pb.idx, torch.int32),
                      (pb.coef, torch.float32)):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("PairBatch: contiguous device tensors (uint8 tables, int32 idx, float32 coef) "
                                 "expected")
        same = pb.keys.shape == pb.locks.shape if kidx is None else \
            (pb.locks.dim() == 3 and pb.keys.dim() == 3 and pb.keys.shape[1:] == pb.locks.shape[1:])
        if not same or tuple(pb.coef.shape) != (self.cfg.batch, 4):
            raise ValueError("PairBatch: lock / key tables of one shape (with key_idx: of one H, W) and "
                             "coef [B, 4] expected")
        xp = None
        if kidx is not None:
            if tuple(kidx.shape) != tuple(pb.idx.shape):
                raise ValueError("PairBatch: key_idx must have idx's shape")
            xp = _lib.mvae_xpairs()
            xp.key_idx = _iptr(kidx)
        p = xp.p if xp is not None else _lib.mvae_pairs()
        p.locks, p.keys = pb.locks.data_ptr(), pb.keys.data_ptr()
        p.height, p.width = int(pb.locks.shape[1]), int(pb.locks.shape[2])
        p.idx, p.coef = pb.idx.data_ptr(), pb.coef.data_ptr()
        p.divisor = 255.0 if pb.normalize else 1.0
        return xp if xp is not None else p

    def _call(self, name: str, x, *args):
        """``mvae_<name>`` on an X tensor, ``mvae_<name>_pairs`` on a ``PairBatch``,
        ``mvae_<name>_xpairs`` on one with a ``key_idx``."""
        xin = self._xin(x)
        if isinstance(xin, _lib.mvae_xpairs):
            return self._check(getattr(self.lib, f"mvae_{name}_xpairs")(self.ctx, C.byref(xin), *args))
        if isinstance(xin, _lib.mvae_pairs):
            return self._check(getattr(self.lib, f"mvae_{name}_pairs")(self.ctx, C.byref(xin), *args))
        return self._check(getattr(self.lib, f"mvae_{name}")(self.ctx, xin, *args))

    def forward(self, x, eps: Optional[torch.Tensor] = None):
        if eps is not None and eps.shape != (3, self.cfg.batch, self.cfg.latent):
            raise ValueError("eps must be [3, B, L] (lock, rotated lock, key)")
        self._call("forward", x, _ptr(eps), self.stream)

    def metric(self, areas: torch.Tensor):
        if areas.shape != (self.cfg.batch,):
            raise ValueError("overlap_areas must be [B]")
        self._check(self.lib.mvae_metric(self.ctx, _ptr(areas), self.stream))

    def backward(self):
        self._check(self.lib.mvae_backward(self.ctx, self.stream))

    @property
    def N_BACKWARD_PARTS(self) -> int:
        """Backward parts of the current schedule (2 + the layer-0 weight-gradient chunks)."""
        return self.lib.mvae_backward_nparts(self.ctx)

    def backward_part(self, part: int):
        """Part ``part`` (0, 1, 2 in order) of ``backward``; see ``grad_ranges``."""
        self._check(self.lib.mvae_backward_part(self.ctx, part, self.stream))

    def grad_ranges(self, part: int):
        """Views of ``grads`` that are final once ``backward_part(part)`` has run."""
        base = self.grads.data_ptr()
        out = []
        for i in range(8):
            p = C.c_void_p()
            n = C.c_size_t()
            if self.lib.mvae_grad_range(self.ctx, part, i, C.byref(p), C.byref(n)) != 0:
                break
            off = (p.value - base) // 4
            if n.value:
                out.append(self.grads[off:off + n.value])
        return out

    def set_option(self, name: str, value: int):
        self._check(self.lib.mvae_set_option(self.ctx, name.encode(), int(value)))

    def adam(self):
        self._check(self.lib.mvae_adam(self.ctx, self.stream))

    def train_step(self, x, areas, eps=None, losses_out=None, dist_out=None):
        if areas.shape != (self.cfg.batch,):
            raise ValueError("overlap_areas must be [B]")
        self._call("train_step", x, _ptr(areas), _ptr(eps), _ptr(losses_out), _ptr(dist_out), self.stream)

    def predict(self, x, eps=None, out=None):
        out = out if out is not None else torch.empty(self.cfg.batch, device=self.dev)
        self._call("predict", x, _ptr(eps), _ptr(out), self.stream)
        return out

    def predict_encode(self, x, eps=None):
        """First phase of ``predict``: encoder + (cosine) the local column sums ``colsq``."""
        self._call("predict_encode", x, _ptr(eps), self.stream)

    def predict_finish(self, out=None):
        """Second phase: distances with the current ``colsq`` (all-reduced under DP)."""
        out = out if out is not None else torch.empty(self.cfg.batch, device=self.dev)
        self._check(self.lib.mvae_predict_finish(self.ctx, _ptr(out), self.stream))
        return out

    def transform(self, x, out=None):
        out = out if out is not None else torch.empty(self.cfg.batch, self.cfg.latent, device=self.dev)
        self._call("transform", x, _ptr(out), self.stream)
        return out

    def reconstruct(self, x, eps=None, out=None):
        out = out if out is not None else torch.empty(self.cfg.batch, self.cfg.D, device=self.dev)
        self._call("reconstruct", x, _ptr(eps), _ptr(out), self.stream)
        return out

    def generate(self, z: torch.Tensor, out=None):
        z = z.reshape(-1, self.cfg.latent).contiguous()
        n = z.shape[0]
        out = out if out is not None else torch.empty(n, self.cfg.D, device=self.dev)
        self._check(self.lib.mvae_generate(self.ctx, _ptr(z), n, _ptr(out), self.stream))
        return out

    # ------------------------------------------------------------------ retrieval
    def embed(self, table: torch.Tensor, idx: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              log_sigma: bool = False, normalize: bool = True):
        """Latent means ``[count, L]`` of single images of a uint8 table ``[n, S, S]``: the images
        ``idx`` (int32, each in ``[0, n)``: the caller's precondition) or all ``n`` in order.
        ``log_sigma``: returns ``(means, log-sigmas)``; then ``out`` is that pair too. ``normalize``:
        pixels / 255, as ``PairBatch``. Any ``count >= 1``: ``ceil(count / 3B)`` encoder passes."""
        if not table.is_cuda or table.dtype != torch.uint8 or table.dim() != 3:
            raise ValueError("embed: a device uint8 table [n, S, S] expected")
        # (a view into a larger storage is fine as long as its images are dense)
        if table.stride() != (table.shape[1] * table.shape[2], table.shape[2], 1):
            raise ValueError("embed: the table's images must be dense (use .contiguous())")
        if idx is not None:
            if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
                raise ValueError("embed: idx must be a contiguous int32 device vector")
        count = int(table.shape[0] if idx is None else idx.shape[0])
        if count < 1:
            raise ValueError("embed: no image to embed")
        L = self.cfg.latent
        mean, ls = (out if log_sigma else (out, None)) if out is not None else (None, None)
        mean = mean if mean is not None else torch.empty(count, L, device=self.dev)
        if log_sigma and ls is None:
            ls = torch.empty(count, L, device=self.dev)
        for t in (mean, ls):
            if t is not None and tuple(t.shape) != (count, L):
                raise ValueError(f"embed: outputs must be [{count}, {L}]")
        im = _lib.mvae_images()
        im.table = table.data_ptr()
        im.height, im.width = int(table.shape[1]), int(table.shape[2])
        im.idx = None if idx is None else idx.data_ptr()
        im.divisor = 255.0 if normalize else 1.0
        self._check(self.lib.mvae_embed_images(self.ctx, C.byref(im), count, _ptr(mean), _ptr(ls), self.stream))
        return (mean, ls) if log_sigma else mean

    def match(self, zl: torch.Tensor, zk: torch.Tensor, k: int, order: int = 1, dist: bool = False, *,
              rl: Optional[torch.Tensor] = None, rk: Optional[torch.Tensor] = None, key_base: int = 0,
              carry=None, target=None, ahead: Optional[torch.Tensor] = None,
              dist_out: Optional[torch.Tensor] = None):
        """The ``k`` best keys of every lock under the model's distance (``cfg.metric``,
        ``cfg.reciprocal``) between embeddings ``zl [N, L]`` and ``zk [M, L]``: ``(values [N, k],
        indices [N, k] int32)``, best first -- ``order`` +1 the largest score, -1 the smallest; ties
        by the smaller index, NaN last. ``dist``: also the whole ``[N, M]`` score matrix.

        A gallery in shards (``mvae_match_ex``; with none of these given the call is ``mvae_match``):
        ``rl`` / ``rk``: the cosine metric's reciprocal column norms ``[L]`` over the whole gallery
        (``match_rnorm(match_colsq(...))``) instead of norms over the rows passed; ``key_base``: the global index of
        ``zk[0]``, which the indices then count from; ``carry=(val, ind)``: the lists of earlier
        shards (disjoint key ranges: the caller's precondition), updated in place to those of the
        union and returned; ``k`` may then exceed ``M`` (empty entries: NaN, index -1).
        ``target=(thr_val [N], thr_idx [N] int32)``: also returns ``ahead [N]`` int32, the number of
        this call's keys strictly before that entry in the order (added to the ``ahead`` given when
        ``carry`` is, else overwritten). ``dist_out``: a ``[N, M]`` float32 view of unit column stride
        (a column block of a wider matrix) the scores are written to; returned like ``dist``."""
        L = self.cfg.latent
        if zl.dim() != 2 or zk.dim() != 2 or zl.shape[1] != L or zk.shape[1] != L:
            raise ValueError(f"match: embeddings must be [N, {L}] and [M, {L}]")
        N, M = int(zl.shape[0]), int(zk.shape[0])
        k = int(k)
        ex = not (rl is None and rk is None and key_base == 0 and carry is None and target is None
                  and ahead is None and dist_out is None)
        if N < 1 or M < 1 or not 1 <= k <= (64 if ex else min(M, 64)):
            raise ValueError("match: N, M >= 1 and 1 <= k <= min(M, 64) expected (k <= 64 for a shard)")
        if order not in (1, -1):
            raise ValueError("match: order must be +1 or -1")
        if not ex:
            val = torch.empty(N, k, device=self.dev)
            ind = torch.empty(N, k, device=self.dev, dtype=torch.int32)
            d = torch.empty(N, M, device=self.dev) if dist else None
            self._check(self.lib.mvae_match(self.ctx, _ptr(zl), N, _ptr(zk), M, k, int(order), _ptr(d), _ptr(val),
                                            ind.data_ptr(), self.stream))
            return (val, ind, d) if dist else (val, ind)
        o = _lib.mvae_match_opts()
        for name, r in (("rl", rl), ("rk", rk)):
            if r is not None and tuple(r.shape) != (L,):
                raise ValueError(f"match: {name} must be [{L}]")
        o.rl, o.rk, o.key_base = _ptr(rl), _ptr(rk), int(key_base)
        if carry is not None:
            val, ind = carry
            o.carry = 1
        else:
            val = torch.empty(N, k, device=self.dev)
            ind = torch.empty(N, k, device=self.dev, dtype=torch.int32)
        if tuple(val.shape) != (N, k) or tuple(ind.shape) != (N, k):
            raise ValueError(f"match: carry must be ([{N}, {k}] float32, [{N}, {k}] int32)")
        d = dist_out if dist_out is not None else (torch.empty(N, M, device=self.dev) if dist else None)
        if d is not None:
            if (not d.is_cuda or d.dtype != torch.float32 or tuple(d.shape) != (N, M) or d.stride(1) != 1
                    or d.stride(0) < M):
                raise ValueError(f"match: dist_out must be a float32 device view [{N}, {M}] of unit column stride")
            o.dist_ld = int(d.stride(0))
        if ahead is not None and target is None:
            raise ValueError("match: ahead needs target=(thr_val, thr_idx)")
        if target is not None:
            tv, ti = target
            ahead = ahead if ahead is not None else torch.zeros(N, device=self.dev, dtype=torch.int32)
            if tuple(tv.shape) != (N,) or tuple(ti.shape) != (N,) or tuple(ahead.shape) != (N,):
                raise ValueError(f"match: target and ahead must be [{N}]")
            o.thr_val, o.thr_idx, o.ahead = _ptr(tv), _iptr(ti), _iptr(ahead)
        self._check(self.lib.mvae_match_ex(self.ctx, _ptr(zl), N, _ptr(zk), M, k, int(order), C.byref(o),
                                           None if d is None else d.data_ptr(), _ptr(val), _iptr(ind), self.stream))
        out = (val, ind) + ((d,) if d is not None else ())
        return out + ((ahead,) if target is not None else ())

    def match_colsq(self, z: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False):
        """Column sums of squares ``[L]`` (float64) of the gallery rows ``z [n, L]``; ``accumulate``:
        added onto ``out``. Shards whose row counts are multiples of 256 (the last one free) give the
        bits of one call over the whole gallery."""
        L = self.cfg.latent
        if z.dim() != 2 or z.shape[1] != L or z.shape[0] < 1:
            raise ValueError(f"match_colsq: a gallery [n, {L}] expected")
        if out is None:
            if accumulate:
                raise ValueError("match_colsq: accumulate needs out")
            out = torch.empty(L, device=self.dev, dtype=torch.float64)
        if not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (L,) or not out.is_contiguous():
            raise ValueError(f"match_colsq: out must be a contiguous float64 device vector [{L}]")
        self._check(self.lib.mvae_match_colsq(self.ctx, _ptr(z), int(z.shape[0]), out.data_ptr(), int(bool(accumulate)),
                                              self.stream))
        return out

    def match_rnorm(self, colsq: torch.Tensor):
        """Reciprocal column norms ``[L]`` (float32) of ``colsq``: what ``match`` takes as ``rl`` / ``rk``."""
        L = self.cfg.latent
        if not colsq.is_cuda or colsq.dtype != torch.float64 or tuple(colsq.shape) != (L,) or not colsq.is_contiguous():
            raise ValueError(f"match_rnorm: a contiguous float64 device vector [{L}] expected")
        out = torch.empty(L, device=self.dev)
        self._check(self.lib.mvae_match_rnorm(self.ctx, colsq.data_ptr(), _ptr(out), self.stream))
        return out

    def pair_scores(self, zl: torch.Tensor, zk: torch.Tensor, rl: Optional[torch.Tensor] = None,
                    rk: Optional[torch.Tensor] = None):
        """``out[i]`` = the score ``match`` gives lock row ``i`` and a key row equal to ``zk[i]`` under
        the same ``rl`` / ``rk``, bit for bit (``None``: norms over the rows passed)."""
        L = self.cfg.latent
        if zl.dim() != 2 or zl.shape[1] != L or zl.shape[0] < 1 or zk.shape != zl.shape:
            raise ValueError(f"pair_scores: two galleries [n, {L}] of equal length expected")
        for r in (rl, rk):
            if r is not None and tuple(r.shape) != (L,):
                raise ValueError(f"pair_scores: rl / rk must be [{L}]")
        out = torch.empty(zl.shape[0], device=self.dev)
        self._check(self.lib.mvae_pair_scores(self.ctx, _ptr(zl), _ptr(zk), int(zl.shape[0]), _ptr(rl), _ptr(rk),
                                              _ptr(out), self.stream))
        return out

    def match_merge(self, vals: torch.Tensor, idx: torch.Tensor, order: int = 1):
        """``vals`` / ``idx [N, parts, k]`` (lists computed apart over disjoint key ranges; empty
        entries: index -1) -> ``(values [N, k], indices [N, k])`` of their union."""
        if vals.dim() != 3 or idx.shape != vals.shape or not 1 <= vals.shape[2] <= 64 or vals.shape[0] < 1 \
                or vals.shape[1] < 1:
            raise ValueError("match_merge: vals / idx [N, parts, k] with 1 <= k <= 64 expected")
        if order not in (1, -1):
            raise ValueError("match_merge: order must be +1 or -1")
        N, parts, k = (int(v) for v in vals.shape)
        val = torch.empty(N, k, device=self.dev)
        ind = torch.empty(N, k, device=self.dev, dtype=torch.int32)
        self._check(self.lib.mvae_match_merge(self.ctx, _ptr(vals), _iptr(idx), N, parts, k, int(order), _ptr(val),
                                              _iptr(ind), self.stream))
        return val, ind

    # ------------------------------------------------------------------ timing regions
    def timing_enable(self, on: bool = True):
        self._check(self.lib.mvae_timing_enable(self.ctx, int(on)))

    def timing_select(self, name: Optional[str] = None):
        """Record only region ``name`` (None: all regions)."""
        r = -1
        if name is not None:
            names = [self.lib.mvae_timing_name(self.ctx, i).decode()
                     for i in range(self.lib.mvae_timing_regions(self.ctx))]
            r = names.index(name)
        self._check(self.lib.mvae_timing_select(self.ctx, r))

    def timing_names(self):
        return [self.lib.mvae_timing_name(self.ctx, i).decode()
                for i in range(self.lib.mvae_timing_regions(self.ctx))]

    def timing_marker(self, name: str, on: bool = True):
        """Bracket region ``name`` with marker kernels (rocprofv3 counter attribution)."""
        self._check(self.lib.mvae_timing_marker(self.ctx, self.timing_names().index(name), int(on)))

    def timing_reset(self):
        self._check(self.lib.mvae_timing_reset(self.ctx))

    def timing_read(self) -> Dict[str, tuple]:
        """Region name -> (total ms, launches) over the HIP events recorded while enabled."""
        out = {}
        tot, cnt = C.c_double(), C.c_int64()
        for r in range(self.lib.mvae_timing_regions(self.ctx)):
            self._check(self.lib.mvae_timing_read(self.ctx, r, C.byref(tot), C.byref(cnt)))
            if cnt.value:
                out[self.lib.mvae_timing_name(self.ctx, r).decode()] = (tot.value, cnt.value)
        return out
