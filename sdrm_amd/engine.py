"""Python handle over the C ABI: owns one `sdrm_engine` and passes torch device pointers through.

torch is used only for device memory and streams (plumbing); every numeric step runs in
libsdrm_hip.so.  Reference lines are into /root/reference/train_SDRM.py."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import weakref

import numpy as np
import torch

from . import _lib, synth


class SdrmError(RuntimeError):
    pass


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Engine.last_plan(): the enumerators of include/sdrm_hip_debug.h (sdrm_debug_last_plan) by name
TRAIN_PATHS = ("per_layer", "skinny", "row96", "row48")
DGRAD_FORMS = ("tiles", "rows_per_layer", "chain", "skinny_own")
SAMPLE_PATHS = ("skinny", "persist", "per_layer")
LastPlan = collections.namedtuple("LastPlan", "train_path parts dgrad sample_path")
# Engine.neumf_rank_problem's record: cols the int32 device view [C]; seen and relevant device CSR tuples (indptr int64 [n_rows + 1], int32
# index view cut to the count, None, (n_rows, C)), rows dense by user id; counts the Python tuple (C, seen's entries, relevant's entries,
# held-out triples dropped for a range defect)
NeumfRankProblem = collections.namedtuple("NeumfRankProblem", "cols seen relevant counts")


class _ParamSpan:
    """What torch.as_tensor needs to wrap foreign device memory: the engine's flat parameter vector."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}


class Engine:
    """eps-predictor SDRM(N_ITEMS=L, EMB_DIM=T, LATENT_DIM=W, n_hidden_layers=H) (:86-95) with its
    Adam state (:309) and DDPM schedule (:296-303) resident on one MI355X."""

    def __init__(self, L, W, T, H, max_rows, device=None):
        if not torch.cuda.is_available():
            raise SdrmError("sdrm_amd needs a ROCm device: no GPU is visible and there is no CPU fallback")
        self.lib = _lib.load()
        self.L, self.W, self.T, self.H, self.max_rows = int(L), int(W), int(T), int(H), int(max_rows)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self._h = C.c_void_p()
        rc = self.lib.sdrm_create(self.L, self.W, self.T, self.H, self.max_rows, self.device.index, C.byref(self._h))
        if rc != 0:
            msg = self.lib.sdrm_last_error(self._h).decode() if self._h else ""
            if self._h:
                self.lib.sdrm_destroy(self._h)
                self._h = C.c_void_p()
            raise SdrmError(f"sdrm_create failed: {_lib.STATUS.get(rc, rc)} {msg}")
        self.P = int(self.lib.sdrm_param_count(self._h))
        assert self.P == synth.param_count(self.L, self.W, self.T, self.H)
        self._sums = torch.zeros(8, dtype=torch.float64, device=self.device)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.gradient_buckets = 2 if os.environ.get("SDRM_AR_BUCKETS", "1").strip() == "2" else 1   # of train_step_sharded
        self._keepalive = None
        self._rank_cache = {}             # rank_metrics, device form: (ks, tp, idcg) per cut-off list
        self._n_views = 0                 # spans handed out by params_view() that some tensor's storage still holds
        self._close_pending = False

    # ------------------------------------------------------------------ plumbing
    def close(self):
        """Frees the engine - unless tensors returned by `params_view()` (an SDRM's `parameters()`) are still alive: they alias the
        master vector sdrm_destroy would free, so the handle then stays allocated (and unused) until the last of them is gone.
        Such a tensor of a closed engine keeps reading the parameters as they were at close()."""
        if not getattr(self, "_h", None):
            return
        if self._n_views > 0:
            self._close_pending = True
            return
        torch.cuda.synchronize(self.device)
        self.lib.sdrm_destroy(self._h)
        self._h = C.c_void_p()
        self._close_pending = False

    @property
    def closed(self):
        return not getattr(self, "_h", None)

    @staticmethod
    def _view_released(eng):
        eng._n_views -= 1
        if eng._close_pending and eng._n_views <= 0:
            eng.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise SdrmError(f"{what}: {_lib.STATUS.get(rc, rc)}: {self.lib.sdrm_last_error(self._h).decode()}")

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=dtype)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype)
        return t.contiguous()

    def _csr_batch(self, who, csr_dev, rows, row0, b):
        """A batch of rows of a `csr_to_device` matrix, `rows` (int64, moved to the device) or row0 .. row0+b-1, as the C ABI takes
        it: (n_rows, n_items, b, the seven leading arguments indptr, indices, data, n_rows, rows, row0, b)."""
        indptr, indices, data, (n_rows, n_items) = csr_dev
        if rows is not None:
            rows = self._dev(rows, torch.int64)
            b = rows.numel()
        elif b is None:
            raise SdrmError(f"{who}: give `rows` or `row0` and `b`")
        if indices.numel() == 0:   # a matrix without an entry: torch gives an empty tensor no address, and the C ABI takes no null array
            indices = indices.new_zeros(1)
        self._feed_keep = (rows, indices)   # what this call made itself, alive until the launch is issued
        return int(n_rows), int(n_items), int(b), (_ptr(indptr), _ptr(indices), _ptr(data), int(n_rows), _ptr(rows), int(row0), int(b))

    def debug_set(self, tile=None, skinny=None, fused_reverse=None, chains=None, nt32_rows=None, nt32_rows_train=None,
                  gradient_buckets=None, rowchain=None, wgrad_strips=None, dgrad_rows=None, rows48=None, rows48_split=None, sample_persist=None, rows48_share=None,
                  csrt_mark=None):
        """Test / tuning hooks of THIS engine (include/sdrm_hip_debug.h): force a GEMM tile shape (-1 = automatic),
        switch the narrow-net kernels, the fused reverse update, the sampler row chains, the 32x32-tile row thresholds,
        the number of gradient all-reduces of the sharded step (1 or 2), the row-owned train forward (0 never, 1 by
        size, 2 whenever the net allows), the strip-owned weight gradients and the row-owned input gradients behind it."""
        if csrt_mark is not None:   # the mark pass of csr_transpose (csrc/csr_transpose.h): 0 by width, 1 global atomics, 2 LDS tiles
            self._check(self.lib.sdrm_debug_set_csrt_mark(self._h, int(csrt_mark)), "sdrm_debug_set_csrt_mark")
        if rowchain is not None:
            self._check(self.lib.sdrm_debug_set_rowchain(self._h, int(rowchain)), "sdrm_debug_set_rowchain")
        if rows48_share is not None:   # the shared-tile form of the 48-row kernels (1 on, 0 the plain form)
            self._check(self.lib.sdrm_debug_set_rows48_share(self._h, int(rows48_share)), "sdrm_debug_set_rows48_share")
        if sample_persist is not None:   # reverse steps in one launch (csrc/sample_persist.h): 0 never, 1 by size, 2 whenever it fits
            self._check(self.lib.sdrm_debug_set_sample_persist(self._h, int(sample_persist)), "sdrm_debug_set_sample_persist")
        if rows48_split is not None:   # column-split row groups of that step: 0 never, 1 by size, 2 / 4 work-groups per group
            self._check(self.lib.sdrm_debug_set_rows48_split(self._h, int(rows48_split)), "sdrm_debug_set_rows48_split")
        if rows48 is not None:   # the same step on 48-row work-groups (csrc/rows48.h): 0 never, 1 by size, 2 whenever the net allows
            self._check(self.lib.sdrm_debug_set_rows48(self._h, int(rows48)), "sdrm_debug_set_rows48")
        if wgrad_strips is not None:
            self._check(self.lib.sdrm_debug_set_wgrad_strips(self._h, int(bool(wgrad_strips))), "sdrm_debug_set_wgrad_strips")
        if dgrad_rows is not None:
            self._check(self.lib.sdrm_debug_set_dgrad_rows(self._h, int(dgrad_rows)), "sdrm_debug_set_dgrad_rows")
        if gradient_buckets is not None:
            self._check(self.lib.sdrm_debug_set_gradient_buckets(self._h, int(gradient_buckets)), "sdrm_debug_set_gradient_buckets")
            self.gradient_buckets = int(gradient_buckets)
        if tile is not None:
            self._check(self.lib.sdrm_debug_set_tile(self._h, int(tile)), "sdrm_debug_set_tile")
        if skinny is not None:
            self._check(self.lib.sdrm_debug_set_skinny(self._h, int(skinny)), "sdrm_debug_set_skinny")
        if fused_reverse is not None:
            self._check(self.lib.sdrm_debug_set_fused_reverse(self._h, int(fused_reverse)), "sdrm_debug_set_fused_reverse")
        if chains is not None:
            self._check(self.lib.sdrm_debug_set_chains(self._h, int(chains)), "sdrm_debug_set_chains")
        if nt32_rows is not None or nt32_rows_train is not None:
            self._check(self.lib.sdrm_debug_set_nt32_rows(self._h, -1 if nt32_rows is None else int(nt32_rows),
                                                          -1 if nt32_rows_train is None else int(nt32_rows_train)),
                        "sdrm_debug_set_nt32_rows")
        return self

    @property
    def sampler_chains(self):
        """Row chains of the sampling call in progress / of the last one (csrc/sdrm_hip.hip: chains_for)."""
        return int(self.lib.sdrm_debug_chains(self._h))

    def last_plan(self):
        """What ran last on this engine (sdrm_debug_last_plan; host-side, nothing is launched): LastPlan(train_path, parts, dgrad,
        sample_path) - the kernel path of the last train forward (one of TRAIN_PATHS), its work-groups per 48-row group (2 / 4:
        column-split), the form of its input gradients (DGRAD_FORMS) and the path of the last sampling call (SAMPLE_PATHS)."""
        v = [C.c_int() for _ in range(4)]
        self._check(self.lib.sdrm_debug_last_plan(self._h, *[C.byref(x) for x in v]), "sdrm_debug_last_plan")
        return LastPlan(TRAIN_PATHS[v[0].value], int(v[1].value), DGRAD_FORMS[v[2].value], SAMPLE_PATHS[v[3].value])

    @property
    def rows48_split_available(self):
        """True when column-split row groups (csrc/rows48.h) may be taken: the net qualifies and the chip maps block b to XCD b & 7."""
        return bool(self.lib.sdrm_debug_rows48_split_available(self._h))

    @property
    def rowchain_available(self):
        """True when this engine's shape qualifies for the row-owned train forward (csrc/rowchain.h)."""
        return bool(self.lib.sdrm_debug_rowchain_available(self._h))

    # ------------------------------------------------------------------ parameters
    def set_params(self, flat):
        flat = self._dev(flat, torch.float32).reshape(-1)
        if flat.numel() != self.P:
            raise SdrmError(f"set_params: expected {self.P} floats, got {flat.numel()}")
        self._check(self.lib.sdrm_set_params(self._h, _ptr(flat), _stream()), "sdrm_set_params")
        self._keepalive = flat

    def _flat_out(self, fn, name):
        out = torch.empty(self.P, dtype=torch.float32, device=self.device)
        self._check(fn(self._h, _ptr(out), _stream()), name)
        return out

    def get_params(self):
        return self._flat_out(self.lib.sdrm_get_params, "sdrm_get_params")

    def params_view(self):
        """The live parameters in place (sdrm_params_ptr): a [P] float32 tensor that ALIASES the engine's master vector - it follows
        every train step without a copy.  Read it; do not write through it (the kernels read compute copies of it)."""
        span = _ParamSpan(int(self.lib.sdrm_params_ptr(self._h)), self.P)
        # torch keeps `span` for the lifetime of the storage it wraps (every view / slice / detach() of the tensor shares that
        # storage); the finalizer holds the engine until the span dies, and close() defers sdrm_destroy while any span is alive
        self._n_views += 1
        weakref.finalize(span, Engine._view_released, self).atexit = False
        return torch.as_tensor(span, device=self.device)

    def philox_draws(self, seed, purpose, step, rows, quads, row0=0, with_bits=True):
        """Test hook (sdrm_debug_philox_draws): the device generator's normals [rows, 4 * quads] and the low three bits of its
        words [rows, 4 * quads] uint8 for (seed, purpose, step)."""
        normals = torch.empty(rows, 4 * quads, dtype=torch.float32, device=self.device)
        bits = torch.empty(rows, 4 * quads, dtype=torch.uint8, device=self.device) if with_bits else None
        self._check(self.lib.sdrm_debug_philox_draws(self._h, int(seed), int(purpose), int(step), int(row0), int(rows), int(quads),
                                                     _ptr(normals), _ptr(bits), _stream()), "sdrm_debug_philox_draws")
        return normals, bits

    def get_grads(self):
        return self._flat_out(self.lib.sdrm_get_grads, "sdrm_get_grads")

    def get_adam_state(self):
        m = torch.empty(self.P, dtype=torch.float32, device=self.device)
        v = torch.empty(self.P, dtype=torch.float32, device=self.device)
        step = C.c_int64()
        self._check(self.lib.sdrm_get_adam_state(self._h, _ptr(m), _ptr(v), C.byref(step), _stream()), "sdrm_get_adam_state")
        return m, v, int(step.value)

    def set_adam_state(self, m, v, step):
        m, v = self._dev(m, torch.float32), self._dev(v, torch.float32)
        self._check(self.lib.sdrm_set_adam_state(self._h, _ptr(m), _ptr(v), int(step), _stream()), "sdrm_set_adam_state")
        self._keepalive = (m, v)

    def adam_reset(self):
        self._check(self.lib.sdrm_adam_reset(self._h, _stream()), "sdrm_adam_reset")

    def set_schedule(self, beta1=1e-4, beta2=0.02):
        self._check(self.lib.sdrm_set_schedule(self._h, beta1, beta2), "sdrm_set_schedule")

    def get_schedule(self):
        n = self.T + 1
        b, a, ab = (np.empty(n, np.float32) for _ in range(3))
        self._check(self.lib.sdrm_get_schedule(self._h, b.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                               ab.ctypes.data_as(C.c_void_p)), "sdrm_get_schedule")
        return b, a, ab

    # ------------------------------------------------------------------ training
    def _randoms(self, noise, t, keep, B):
        noise = self._dev(noise, torch.float32)
        t = self._dev(t, torch.int64)
        keep = self._dev(keep, torch.uint8)
        if tuple(noise.shape) != (B, self.L) or tuple(t.shape) != (B,) or tuple(keep.shape) != (3, B, self.L):
            raise SdrmError("explicit randoms: expected noise [B,L], t [B], keep [3,B,L]")
        self._keepalive = (noise, t, keep)
        return _lib.TrainRandoms(noise.data_ptr(), t.data_ptr(), keep.data_ptr())

    def train_forward(self, x0, noise=None, t=None, keep=None, seed=0, step=0, nd=1.0, row0=0, sums=None):
        """Phase 1 (:326-333 up to the loss sums).  Explicit randoms if `noise` is given, else Philox."""
        x0 = self._dev(x0, torch.float32)
        B = x0.shape[0]
        if x0.dim() != 2 or x0.shape[1] != self.L:
            raise SdrmError(f"train_forward: x0 must be [B,{self.L}]")
        self._x0 = x0
        sums = self._sums if sums is None else sums
        if noise is not None:
            rnd = self._randoms(noise, t, keep, B)
            rc = self.lib.sdrm_train_forward(self._h, _ptr(x0), B, int(row0), _lib.RNG_EXPLICIT, C.byref(rnd), 0, 0,
                                             float(nd), _ptr(sums), _stream())
        else:
            rc = self.lib.sdrm_train_forward(self._h, _ptr(x0), B, int(row0), _lib.RNG_PHILOX, None, int(seed),
                                             int(step), float(nd), _ptr(sums), _stream())
        self._check(rc, "sdrm_train_forward")
        return sums

    def train_backward(self, sums=None, grad=None):
        """Phase 2: seeds from the (global) sums, backward, flat gradient.  Returns the device loss scalar."""
        sums = self._sums if sums is None else sums
        self._check(self.lib.sdrm_train_backward(self._h, _ptr(sums), _ptr(grad), _ptr(self._loss), _stream()),
                    "sdrm_train_backward")
        return self._loss

    def train_backward_begin(self, sums=None, grad=None):
        """Phase 2, first call: on return the FIRST bucket of `grad` (see `grad_buckets`) is final in stream order;
        the upper layers' weight gradients are left to `train_backward_finish`."""
        sums = self._sums if sums is None else sums
        self._check(self.lib.sdrm_train_backward_begin(self._h, _ptr(sums), _ptr(grad), _ptr(self._loss), _stream()),
                    "sdrm_train_backward_begin")
        return self._loss

    def train_backward_finish(self, grad=None):
        """Phase 2, second call: upper-layer weight gradients, then the SECOND bucket is final."""
        self._check(self.lib.sdrm_train_backward_finish(self._h, _ptr(grad), _stream()), "sdrm_train_backward_finish")

    def grad_buckets(self):
        """((offset, length) of the first bucket, (offset, length) of the second) in the flat gradient."""
        v = [C.c_int64() for _ in range(4)]
        self._check(self.lib.sdrm_grad_buckets(self._h, *[C.byref(x) for x in v]), "sdrm_grad_buckets")
        return (int(v[0].value), int(v[1].value)), (int(v[2].value), int(v[3].value))

    def adam_step(self, lr, grad=None):
        """Phase 3: coupled-L2 Adam (:309,:337) at the caller's per-epoch lr (:316)."""
        self._check(self.lib.sdrm_adam_step(self._h, _ptr(grad), float(lr), _stream()), "sdrm_adam_step")

    def train_step(self, x0, lr, noise=None, t=None, keep=None, seed=0, step=0, nd=1.0):
        """One whole step (:326-337) on this GPU; returns the device loss scalar (no host sync, Q14)."""
        x0 = self._dev(x0, torch.float32)
        B = x0.shape[0]
        if x0.dim() != 2 or x0.shape[1] != self.L:
            raise SdrmError(f"train_step: x0 must be [B,{self.L}]")
        self._x0 = x0
        if noise is not None:
            rnd = self._randoms(noise, t, keep, B)
            rc = self.lib.sdrm_train_step(self._h, _ptr(x0), B, float(lr), _lib.RNG_EXPLICIT, C.byref(rnd), 0, 0,
                                          float(nd), _ptr(self._loss), _stream())
        else:
            rc = self.lib.sdrm_train_step(self._h, _ptr(x0), B, float(lr), _lib.RNG_PHILOX, None, int(seed), int(step),
                                          float(nd), _ptr(self._loss), _stream())
        self._check(rc, "sdrm_train_step")
        return self._loss

    # ------------------------------------------------------------------ multi-GPU exchange inside the library
    @staticmethod
    def comm_available() -> bool:
        """True when librccl resolves in this process (a local check: agree on it across ranks BEFORE comm_init_rank)."""
        return bool(_lib.load().sdrm_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL unique id (rank 0 calls this and ships the bytes to the other ranks by any channel)."""
        buf = C.create_string_buffer(128)
        rc = _lib.load().sdrm_comm_unique_id(buf)
        if rc != 0:
            raise SdrmError(f"sdrm_comm_unique_id: {_lib.STATUS.get(rc, rc)} (librccl could not be loaded?)")
        return buf.raw

    def comm_init_rank(self, nranks: int, rank: int, unique_id: bytes):
        """Joins the RCCL communicator of the user-sharded step (the library owns it)."""
        if len(unique_id) != 128:
            raise SdrmError("comm_init_rank: the unique id is 128 bytes")
        self._check(self.lib.sdrm_comm_init_rank(self._h, int(nranks), int(rank), C.c_char_p(unique_id)), "sdrm_comm_init_rank")
        return self

    def comm_info(self):
        n, r = C.c_int(), C.c_int()
        self._check(self.lib.sdrm_comm_info(self._h, C.byref(n), C.byref(r)), "sdrm_comm_info")
        return int(n.value), int(r.value)

    def train_step_sharded(self, x0, lr, row0=0, noise=None, t=None, keep=None, seed=0, step=0, nd=1.0):
        """One step on this rank's rows with both exchanges (loss sums, gradient buckets) issued by the library over
        RCCL; returns the device scalar holding the GLOBAL loss."""
        x0 = self._dev(x0, torch.float32)
        B = x0.shape[0]
        if x0.dim() != 2 or x0.shape[1] != self.L:
            raise SdrmError(f"train_step_sharded: x0 must be [B,{self.L}]")
        self._x0 = x0
        if noise is not None:
            rnd = self._randoms(noise, t, keep, B)
            rc = self.lib.sdrm_train_step_sharded(self._h, _ptr(x0), B, int(row0), float(lr), _lib.RNG_EXPLICIT, C.byref(rnd),
                                                  0, 0, float(nd), _ptr(self._loss), _stream())
        else:
            rc = self.lib.sdrm_train_step_sharded(self._h, _ptr(x0), B, int(row0), float(lr), _lib.RNG_PHILOX, None, int(seed),
                                                  int(step), float(nd), _ptr(self._loss), _stream())
        self._check(rc, "sdrm_train_step_sharded")
        return self._loss

    def train_outputs(self, B):
        out = torch.empty(3, B, self.L, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_get_train_outputs(self._h, _ptr(out), _stream()), "sdrm_get_train_outputs")
        return out

    def staged(self, B):
        """Test hook (sdrm_debug_get_staged): what the last train forward staged - the layer-0 inputs [3,B,L] of the P, S and Q
        pass in user order, and the users' timesteps [B] int32."""
        out = torch.empty(3, B, self.L, dtype=torch.float32, device=self.device)
        t = torch.empty(B, dtype=torch.int32, device=self.device)
        self._check(self.lib.sdrm_debug_get_staged(self._h, _ptr(out), _ptr(t), _stream()), "sdrm_debug_get_staged")
        return out, t

    def preacts(self, layer, B):
        """Pre-activations [3,B,W] of layer `layer` from the last train forward (parity tests)."""
        out = torch.empty(3, B, self.W, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_get_preacts(self._h, int(layer), _ptr(out), _stream()), "sdrm_get_preacts")
        return out

    def launch_count(self):
        """Kernel launches issued through this handle so far (bench.py: launches per step)."""
        return int(self.lib.sdrm_launch_count(self._h))

    # ------------------------------------------------------------------ profiling (bench only)
    def profile_begin(self, capacity=4096, only=None):
        """`only`: name of the one kernel class to bracket (as `profile_end` returns them); None = every GEMM launch."""
        cls = -1
        if only is not None:
            names = [self.lib.sdrm_profile_name(c).decode() for c in range(self.lib.sdrm_profile_classes())]
            cls = names.index(only)
        self._check(self.lib.sdrm_profile_only(self._h, cls), "sdrm_profile_only")
        self._check(self.lib.sdrm_profile_begin(self._h, int(capacity)), "sdrm_profile_begin")

    def profile_end(self):
        """Returns {kernel class name: (total_ms, launches, algorithmic_flops)} for classes that ran."""
        self._check(self.lib.sdrm_profile_end(self._h, _stream()), "sdrm_profile_end")
        out = {}
        for c in range(self.lib.sdrm_profile_classes()):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            self._check(self.lib.sdrm_profile_get(self._h, c, C.byref(ms), C.byref(n), C.byref(fl)), "sdrm_profile_get")
            if n.value:
                out[self.lib.sdrm_profile_name(c).decode()] = (ms.value, int(n.value), fl.value)
        return out

    # ------------------------------------------------------------------ inference
    def forward(self, x, t, keep=None, seed=0, step=0, row0=0):
        """SDRM.forward(x, t) (:97-103); dropout is always on (Q2)."""
        x = self._dev(x, torch.float32)
        t = self._dev(t, torch.int64)
        n = x.shape[0]
        out = torch.empty(n, self.L, dtype=torch.float32, device=self.device)
        if keep is not None:
            keep = self._dev(keep, torch.uint8)
            rc = self.lib.sdrm_forward(self._h, _ptr(x), _ptr(t), n, _lib.RNG_EXPLICIT, _ptr(keep), 0, 0, 0, _ptr(out),
                                       _stream())
        else:
            rc = self.lib.sdrm_forward(self._h, _ptr(x), _ptr(t), n, _lib.RNG_PHILOX, None, int(seed), int(step),
                                       int(row0), _ptr(out), _stream())
        self._check(rc, "sdrm_forward")
        self._keepalive = (x, t, keep)
        return out

    def sample(self, n, nd=1.0, multires=False, xT=None, z=None, keep=None, Tj=None, seed=0, call_id=0, row0=0,
               return_Tj=False):
        """Latent part of sample_ddpm (:37-59): returns x_0 latents [n,L] (caller applies vae.decode)."""
        out = torch.empty(n, self.L, dtype=torch.float32, device=self.device)
        tj_out = torch.zeros(n, dtype=torch.int64, device=self.device) if (multires and return_Tj) else None
        if xT is not None:
            xT, z, keep = self._dev(xT, torch.float32), self._dev(z, torch.float32), self._dev(keep, torch.uint8)
            Tj = None if Tj is None else self._dev(Tj, torch.int64)
            if tuple(z.shape) != (self.T + 1, n, self.L) or tuple(keep.shape) != (self.T + 1, n, self.L):
                raise SdrmError("sample: z and keep must be [T+1,n,L]")
            rc = self.lib.sdrm_sample(self._h, n, float(nd), int(bool(multires)), _lib.RNG_EXPLICIT, _ptr(xT), _ptr(z),
                                      _ptr(keep), _ptr(Tj), 0, 0, 0, _ptr(out), _ptr(tj_out), _stream())
        else:
            rc = self.lib.sdrm_sample(self._h, n, float(nd), int(bool(multires)), _lib.RNG_PHILOX, None, None, None,
                                      None, int(seed), int(call_id), int(row0), _ptr(out), _ptr(tj_out), _stream())
        self._check(rc, "sdrm_sample")
        self._keepalive = (xT, z, keep, Tj)
        return (out, tj_out) if return_Tj else out

    def sample_begin(self, n, nd=1.0, multires=False, seed=0, call_id=0, row0=0):
        """Resumable PHILOX-mode sampler (bench.py interleaves its steps with train steps)."""
        self._check(self.lib.sdrm_sample_begin(self._h, int(n), float(nd), int(bool(multires)), _lib.RNG_PHILOX, None,
                                               None, None, None, int(seed), int(call_id), int(row0), None, _stream()),
                    "sdrm_sample_begin")
        self._sample_n = int(n)

    def sample_steps(self, count):
        self._check(self.lib.sdrm_sample_steps(self._h, int(count), _stream()), "sdrm_sample_steps")
        return int(self.lib.sdrm_sample_remaining(self._h))

    def sample_end(self):
        out = torch.empty(self._sample_n, self.L, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_sample_end(self._h, _ptr(out), _stream()), "sdrm_sample_end")
        return out

    def reverse_step(self, x, i, z, keep):
        x = self._dev(x, torch.float32).clone()
        z = None if z is None else self._dev(z, torch.float32)
        keep = self._dev(keep, torch.uint8)
        self._check(self.lib.sdrm_reverse_step(self._h, _ptr(x), x.shape[0], int(i), _ptr(z), _ptr(keep), _stream()),
                    "sdrm_reverse_step")
        self._keepalive = (z, keep)
        return x

    def equal_sparsity(self, raw, sparsity, return_threshold=False):
        """main.py:177-180 on the device: `(raw >= np.quantile(raw.flatten(), sparsity))` as a uint8 tensor of raw's shape
        (and the float32 threshold np.quantile returns, as a 0-d device tensor, when asked)."""
        raw = self._dev(raw, torch.float32)
        out = torch.empty(raw.shape, dtype=torch.uint8, device=self.device)
        thr = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_equal_sparsity(self._h, _ptr(raw), raw.numel(), float(sparsity), _ptr(out), _ptr(thr),
                                                 _stream()), "sdrm_equal_sparsity")
        return (out, thr) if return_threshold else out

    _CSR_SIDES = {">=": 0, "<=": 1}

    def equal_sparsity_csr_begin(self, raw, sparsity, side=">="):
        """First half of `equal_sparsity_csr` (`sdrm_equal_sparsity_csr_begin`): threshold, bit mask and indptr on the device, one
        stream synchronise, nnz on the host.  Returns (indptr int64 [n_rows + 1], nnz, threshold 0-d float32)."""
        if side not in self._CSR_SIDES:
            raise SdrmError(f"equal_sparsity_csr: side must be '>=' or '<=', got {side!r}")
        raw = self._dev(raw, torch.float32)
        if raw.dim() != 2:
            raise SdrmError(f"equal_sparsity_csr: SDRM_ERR_SHAPE: raw must be 2-D, got {tuple(raw.shape)}")
        indptr = torch.empty(raw.shape[0] + 1, dtype=torch.int64, device=self.device)
        thr = torch.empty((), dtype=torch.float32, device=self.device)
        nnz = C.c_int64(-1)
        self._check(self.lib.sdrm_equal_sparsity_csr_begin(self._h, _ptr(raw), raw.shape[0], raw.shape[1], float(sparsity),
                                                           self._CSR_SIDES[side], _ptr(indptr), _ptr(thr), C.byref(nnz), _stream()),
                    "sdrm_equal_sparsity_csr_begin")
        return indptr, int(nnz.value), thr

    def equal_sparsity_csr_end(self, indices):
        """Second half: fills `indices` (int32 device tensor of at least nnz elements) from the pending mask."""
        if indices.dtype != torch.int32 or not indices.is_contiguous() or indices.device != self.device:
            raise SdrmError("equal_sparsity_csr_end: indices must be a contiguous int32 tensor on the engine's device")
        self._check(self.lib.sdrm_equal_sparsity_csr_end(self._h, _ptr(indices), indices.numel(), _stream()), "sdrm_equal_sparsity_csr_end")
        return indices

    def equal_sparsity_csr(self, raw, sparsity, side=">=", return_threshold=False):
        """main.py:177-180 (`side=">="`) or the NeuMF branch's other tail, main.py:260 (`side="<="`), as a canonical CSR matrix made on
        the device: (indptr int64 [n_rows + 1], indices int32 [nnz], shape) as device tensors - columns ascend within a row, no data
        array (all ones, as `csr_to_device` returns for such a matrix) - and the float32 threshold when asked.  `raw` is 2-D, on the
        device or the host.  No dense 0/1 matrix exists; the one readback is nnz (8 bytes)."""
        shape = tuple(int(v) for v in raw.shape)
        indptr, nnz, thr = self.equal_sparsity_csr_begin(raw, sparsity, side)
        indices = self.equal_sparsity_csr_end(torch.empty(nnz, dtype=torch.int32, device=self.device))
        out = (indptr, indices, shape)
        return (out, thr) if return_threshold else out

    # ------------------------------------------------------------------ VAE decode on the engine
    def _decoder(self, w1, b1, w2, b2):
        w1, b1, w2, b2 = (self._dev(t.detach() if isinstance(t, torch.Tensor) else t, torch.float32) for t in (w1, b1, w2, b2))
        hidden, latent = w1.shape
        n_items = w2.shape[0]
        if tuple(b1.shape) != (hidden,) or tuple(w2.shape) != (n_items, hidden) or tuple(b2.shape) != (n_items,):
            raise SdrmError("vae_decode: expected decoder[0].weight [hidden, latent], .bias [hidden], decoder[2].weight [items, hidden], .bias [items]")
        self._keepalive = (w1, b1, w2, b2)
        return _lib.VaeDecoder(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), latent, hidden, n_items), latent, n_items

    def vae_decode(self, z, w1, b1, w2, b2):
        """`VAE.decode(z)` (train_SDRM.py:252-254) for decoder = Linear -> Tanh -> Linear given as its four tensors."""
        dec, latent, n_items = self._decoder(w1, b1, w2, b2)
        z = self._dev(z, torch.float32)
        if z.dim() != 2 or z.shape[1] != latent:
            raise SdrmError(f"vae_decode: z must be [n,{latent}]")
        out = torch.empty(z.shape[0], n_items, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_vae_decode(self._h, C.byref(dec), _ptr(z), z.shape[0], _ptr(out), _stream()), "sdrm_vae_decode")
        return out

    # ------------------------------------------------------------------ VAE encode on the engine (frozen, eval mode)
    def vae_encoder_load(self, w1, b1, w2, b2):
        """Stages the frozen encoder `Linear(n_items, hidden) -> Tanh -> Linear(hidden, 2 latent)` (train_SDRM.py:210-212) given as
        its four tensors; the engine keeps its own copies.  A second load replaces the first."""
        w1, b1, w2, b2 = (self._dev(t.detach() if isinstance(t, torch.Tensor) else t, torch.float32) for t in (w1, b1, w2, b2))
        if w1.dim() != 2 or w2.dim() != 2 or w2.shape[0] % 2:
            raise SdrmError("vae_encoder_load: expected encoder[0].weight [hidden, items] and encoder[2].weight [2 latent, hidden]")
        hidden, n_items = w1.shape
        latent = w2.shape[0] // 2
        if tuple(b1.shape) != (hidden,) or tuple(w2.shape) != (2 * latent, hidden) or tuple(b2.shape) != (2 * latent,):
            raise SdrmError("vae_encoder_load: expected encoder[0].weight [hidden, items], .bias [hidden], encoder[2].weight [2 latent, hidden], .bias [2 latent]")
        enc = _lib.VaeEncoder(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), n_items, hidden, latent)
        self._check(self.lib.sdrm_vae_encoder_load(self._h, C.byref(enc), _stream()), "sdrm_vae_encoder_load")
        self._keepalive = (w1, b1, w2, b2)
        self._encoder = (int(n_items), int(hidden), int(latent))

    def _encoder_dims(self, who):
        enc = getattr(self, "_encoder", None)
        if enc is None:
            raise SdrmError(f"{who}: SDRM_ERR_STATE: no encoder loaded (vae_encoder_load)")
        return enc

    def _kl_out(self, return_kl):
        return torch.empty((), dtype=torch.float32, device=self.device) if return_kl else None

    def vae_encode(self, x, return_kl=False):
        """`VAE.encode(x)` in eval mode (train_SDRM.py:241-250) for a dense x [n, n_items]: z = mu [n, latent] (and the kl as a 0-d
        device tensor when asked).  A width other than the loaded encoder's raises SdrmError (SDRM_ERR_SHAPE): the C call takes none."""
        n_items, _, latent = self._encoder_dims("sdrm_vae_encode")
        x = self._dev(x, torch.float32)
        if x.dim() != 2 or x.shape[1] != n_items:
            raise SdrmError(f"sdrm_vae_encode: SDRM_ERR_SHAPE: x must be [n,{n_items}], got {tuple(x.shape)}")
        z = torch.empty(x.shape[0], latent, dtype=torch.float32, device=self.device)
        kl = self._kl_out(return_kl)
        self._check(self.lib.sdrm_vae_encode(self._h, _ptr(x), x.shape[0], _ptr(z), _ptr(kl), _stream()), "sdrm_vae_encode")
        return (z, kl) if return_kl else z

    def vae_encode_csr(self, csr_dev, rows=None, row0=0, b=None, return_kl=False, check=True):
        """The same z straight from the rows `rows` (or row0 .. row0+b-1) of a `csr_to_device` matrix: the first Linear is a gather
        of W1's columns, no dense batch exists.  Range checks and `check` as in `csr_rows_to_dense`."""
        n_items, _, latent = self._encoder_dims("sdrm_vae_encode_csr")
        _, width, b, batch = self._csr_batch("vae_encode_csr", csr_dev, rows, row0, b)
        if width != n_items:
            raise SdrmError(f"sdrm_vae_encode_csr: SDRM_ERR_SHAPE: the matrix has {width} columns, the encoder {n_items}")
        z = torch.empty(b, latent, dtype=torch.float32, device=self.device)
        kl = self._kl_out(return_kl)
        self._check(self.lib.sdrm_vae_encode_csr(self._h, *batch, _ptr(z), _ptr(kl), _stream()), "sdrm_vae_encode_csr")
        if check:
            self.feed_status()
        return (z, kl) if return_kl else z

    # ------------------------------------------------------------------ loss head of the VAE pre-stage (csrc/nll.h)
    def _nll_batch(self, who, logits, csr_dev, rows, row0, b):
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device != self.device or not logits.is_contiguous():
            raise SdrmError(f"{who}: logits must be a contiguous float32 tensor on the engine's device")
        _, n_items, b, batch = self._csr_batch(who, csr_dev, rows, row0, b)
        if logits.dim() != 2 or tuple(logits.shape) != (b, n_items):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: logits must be [{b},{n_items}], got {tuple(logits.shape)}")
        return n_items, b, batch

    def multinomial_nll_csr(self, logits, csr_dev, rows=None, row0=0, b=None, check=True):
        """train_SDRM.py:141-142 on the device, `-mean(sum(log_softmax(logits) * X))` for the X whose rows are the rows `rows` (or
        row0 .. row0+b-1) of a `csr_to_device` matrix: (loss 0-d float32, lse [b] float32) as device tensors; no dense X exists and
        nothing is read back.  Range checks and `check` as in `csr_rows_to_dense`."""
        n_items, b, batch = self._nll_batch("multinomial_nll_csr", logits, csr_dev, rows, row0, b)
        lse = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_multinomial_nll_csr(self._h, _ptr(logits), *batch, n_items, _ptr(lse), _ptr(loss), _stream()),
                    "sdrm_multinomial_nll_csr")
        if check:
            self.feed_status()
        return loss, lse

    def multinomial_nll_csr_grad(self, logits, lse, csr_dev, rows=None, row0=0, b=None, scale=None, out=None):
        """Its gradient with respect to the logits, `scale * (softmax(logits) * X.sum(1) - X) / b` [b, n_items], from the `lse` the
        forward returned.  `scale`: a float32 device tensor of one element (the upstream gradient; None = 1).  `out=logits` writes it
        in place of the logits; any other `out` must not overlap them.  The range checks land in the status word `feed_status` reads."""
        n_items, b, batch = self._nll_batch("multinomial_nll_csr_grad", logits, csr_dev, rows, row0, b)
        for name, t, n in (("lse", lse, b), ("scale", scale, 1)):
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or t.numel() != n or not t.is_contiguous()):
                raise SdrmError(f"multinomial_nll_csr_grad: {name} must be a contiguous float32 device tensor of {n} element(s)")
        if out is None:
            out = torch.empty_like(logits)
        elif out.dtype != torch.float32 or out.device != self.device or out.shape != logits.shape or not out.is_contiguous():
            raise SdrmError("multinomial_nll_csr_grad: out must be a contiguous float32 device tensor of the logits' shape")
        self._check(self.lib.sdrm_multinomial_nll_csr_grad(self._h, _ptr(logits), _ptr(lse), *batch, n_items, _ptr(scale), _ptr(out), _stream()),
                    "sdrm_multinomial_nll_csr_grad")
        return out

    # ------------------------------------------------------------------ train-mode input layer of the VAE encoder (csrc/input_layer.h)
    def _f32(self, who, name, t, shape):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
            raise SdrmError(f"{who}: {name} must be a contiguous float32 tensor on the engine's device")
        if tuple(t.shape) != tuple(shape):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {name} must be {list(shape)}, got {list(t.shape)}")
        return t

    def _index(self, who, name, t, dtype, n):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.numel() != n:
            raise SdrmError(f"{who}: {name} must be a contiguous {dtype} tensor of {n} element(s) on the engine's device")
        return t

    def vae_input_layer_fwd(self, w1, b1, csr_dev, rows=None, row0=0, b=None, seed=0, step=0, p_drop=0.5, check=True):
        """train_SDRM.py:242-244 up to the first pre-activation, in train mode, from the rows `rows` (or row0 .. row0+b-1) of a
        `csr_to_device` matrix: (pre [b, hidden], rowscale [b]) float32 device tensors for w1 [hidden, n_items], b1 [hidden] as
        `nn.Linear` holds them.  The dropout bits are the engine's Philox draws of (seed, step, feed row, column), not torch's.
        Range checks and `check` as in `csr_rows_to_dense`."""
        who = "vae_input_layer_fwd"
        _, n_items, b, batch = self._csr_batch(who, csr_dev, rows, row0, b)
        if not isinstance(w1, torch.Tensor) or w1.dim() != 2:
            raise SdrmError(f"{who}: w1 must be a 2-D tensor [hidden, n_items]")
        hidden = int(w1.shape[0])
        w1 = self._f32(who, "w1", w1, (hidden, n_items))
        b1 = self._f32(who, "b1", b1, (hidden,))
        pre = torch.empty(b, hidden, dtype=torch.float32, device=self.device)
        rowscale = torch.empty(b, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_vae_input_layer_fwd(self._h, _ptr(w1), _ptr(b1), n_items, hidden, *batch, int(seed) & (2 ** 64 - 1),
                                                      int(step) & 0xFFFFFFFF, float(p_drop), _ptr(pre), _ptr(rowscale), _stream()),
                    "sdrm_vae_input_layer_fwd")
        if check:
            self.feed_status()
        return pre, rowscale

    def vae_input_layer_wgrad(self, dpre, rowscale, csc_dev, pos=None, lo=0, b=None, seed=0, step=0, p_drop=0.5, out=None, check=True):
        """The weight gradient of that Linear, dW1 [hidden, n_items], for dpre [b, hidden] and the `rowscale` the forward returned,
        from a `csc_to_device` matrix: the batch is the feed rows R with 0 <= pos[R] - lo < b (`pos` int32 [n_rows], the inverse of
        the epoch's order; None: rows lo .. lo+b-1).  Every element of the result is written once - `out` needs no zeroing."""
        who = "vae_input_layer_wgrad"
        colptr, rowidx, data, (n_rows, n_items) = csc_dev
        if not isinstance(dpre, torch.Tensor) or dpre.dim() != 2:
            raise SdrmError(f"{who}: dpre must be a 2-D tensor [b, hidden]")
        b = int(dpre.shape[0]) if b is None else int(b)
        hidden = int(dpre.shape[1])
        dpre = self._f32(who, "dpre", dpre, (b, hidden))
        rowscale = self._f32(who, "rowscale", rowscale, (b,))
        if pos is not None:
            pos = self._index(who, "pos", pos, torch.int32, int(n_rows))
        if rowidx.numel() == 0:
            rowidx = rowidx.new_zeros(1)
        if out is None:
            out = torch.empty(hidden, int(n_items), dtype=torch.float32, device=self.device)
        else:
            out = self._f32(who, "out", out, (hidden, int(n_items)))
        self._check(self.lib.sdrm_vae_input_layer_wgrad(self._h, _ptr(dpre), _ptr(rowscale), hidden, _ptr(colptr), _ptr(rowidx), _ptr(data),
                                                        int(n_rows), int(n_items), _ptr(pos), int(lo), b, int(seed) & (2 ** 64 - 1),
                                                        int(step) & 0xFFFFFFFF, float(p_drop), _ptr(out), _stream()), "sdrm_vae_input_layer_wgrad")
        if check:
            self.feed_status()
        return out

    # ------------------------------------------------------------------ train-mode latent head of the VAE encoder (csrc/latent.h)
    def vae_latent_fwd(self, pre, w2, b2, rows=None, row0=0, seed=0, step=0, eps=None):
        """train_SDRM.py:244-250 behind the first pre-activation, in train mode: (z [b, latent], kl 0-d, saved) float32 device tensors
        for pre [b, hidden] (what `vae_input_layer_fwd` left), w2 [2 latent, hidden], b2 [2 latent] as `nn.Linear` holds them.
        `eps=None` draws the reparameterisation noise on the device, the engine's Philox draw of (seed, step, feed row, column) with the
        feed rows `rows` (int64) or row0 .. row0+b-1 - not torch's generator; a given float32 [b, latent] device tensor is used as it
        is and not written.  `saved` = (h1, out2, eps) is what `vae_latent_bwd` takes; nothing is read back."""
        who = "vae_latent_fwd"
        if not isinstance(pre, torch.Tensor) or pre.dim() != 2 or not isinstance(w2, torch.Tensor) or w2.dim() != 2 or w2.shape[0] % 2:
            raise SdrmError(f"{who}: pre must be a 2-D tensor [b, hidden] and w2 a 2-D tensor [2 latent, hidden]")
        b, hidden, latent = int(pre.shape[0]), int(pre.shape[1]), int(w2.shape[0]) // 2
        pre = self._f32(who, "pre", pre, (b, hidden))
        w2 = self._f32(who, "w2", w2, (2 * latent, hidden))
        b2 = self._f32(who, "b2", b2, (2 * latent,))
        if rows is not None:
            rows = self._index(who, "rows", rows, torch.int64, b)
        draw = eps is None
        eps = torch.empty(b, latent, dtype=torch.float32, device=self.device) if draw else self._f32(who, "eps", eps, (b, latent))
        h1 = torch.empty(b, hidden, dtype=torch.float32, device=self.device)
        out2 = torch.empty(b, 2 * latent, dtype=torch.float32, device=self.device)
        z = torch.empty(b, latent, dtype=torch.float32, device=self.device)
        kl = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_vae_latent_fwd(self._h, _ptr(pre), _ptr(w2), _ptr(b2), hidden, latent, _ptr(rows), int(row0), b,
                                                 int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(draw), _ptr(h1), _ptr(out2), _ptr(eps),
                                                 _ptr(z), _ptr(kl), _stream()), "sdrm_vae_latent_fwd")
        return z, kl, (h1, out2, eps)

    def vae_latent_bwd(self, saved, w2, gz, gkl, out=None):
        """Its backward: (dpre [b, hidden], dw2 [2 latent, hidden], db2 [2 latent]) for `saved` as the forward returned it, the w2 that
        forward read, and the upstream gradients gz [b, latent] and gkl (a float32 device tensor of ONE element) - either may be None,
        which means zero.  Every element of the three results is written once: `out` = (dpre, dw2, db2) needs no zeroing."""
        who = "vae_latent_bwd"
        if not isinstance(saved, (tuple, list)) or len(saved) != 3 or not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in saved):
            raise SdrmError(f"{who}: saved must be the (h1, out2, eps) a vae_latent_fwd returned")
        h1, out2, eps = saved
        b, hidden, latent = int(h1.shape[0]), int(h1.shape[1]), int(eps.shape[1])
        h1 = self._f32(who, "h1", h1, (b, hidden))
        out2 = self._f32(who, "out2", out2, (b, 2 * latent))
        eps = self._f32(who, "eps", eps, (b, latent))
        w2 = self._f32(who, "w2", w2, (2 * latent, hidden))
        if gz is not None:
            gz = self._f32(who, "gz", gz, (b, latent))
        if gkl is not None and (not isinstance(gkl, torch.Tensor) or gkl.dtype != torch.float32 or gkl.device != self.device or gkl.numel() != 1):
            raise SdrmError(f"{who}: gkl must be a float32 device tensor of 1 element")
        shapes = ((b, hidden), (2 * latent, hidden), (2 * latent,))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        else:
            out = tuple(self._f32(who, name, t, s) for name, t, s in zip(("dpre", "dw2", "db2"), out, shapes))
        self._check(self.lib.sdrm_vae_latent_bwd(self._h, _ptr(h1), _ptr(out2), _ptr(eps), _ptr(w2), hidden, latent, b, _ptr(gz), _ptr(gkl),
                                                 _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()), "sdrm_vae_latent_bwd")
        return out

    # ------------------------------------------------------------------ train-mode decoder and loss head (csrc/decoder_train.h)
    def _decoder_head(self, who, z, w3, b3, w4, b4, csr_dev, rows, row0, b):
        _, n_items, b, batch = self._csr_batch(who, csr_dev, rows, row0, b)
        if not isinstance(w3, torch.Tensor) or w3.dim() != 2:
            raise SdrmError(f"{who}: w3 must be a 2-D tensor [hidden, latent]")
        hidden, latent = int(w3.shape[0]), int(w3.shape[1])
        z = self._f32(who, "z", z, (b, latent))
        w3 = self._f32(who, "w3", w3, (hidden, latent))
        b3 = self._f32(who, "b3", b3, (hidden,))
        w4 = self._f32(who, "w4", w4, (n_items, hidden))
        b4 = self._f32(who, "b4", b4, (n_items,))
        dec = _lib.VaeDecoder(w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(), latent, hidden, n_items)
        return dec, z, (b, latent, hidden, n_items), batch

    def vae_decoder_nll_fwd(self, z, w3, b3, w4, b4, csr_dev, rows=None, row0=0, b=None, check=True):
        """train_SDRM.py:252-254 and :141-142 in train mode: `-mean(sum(log_softmax(decoder(z)) * X))` for z [b, latent], the decoder's
        four tensors w3 [hidden, latent], b3 [hidden], w4 [n_items, hidden], b4 [n_items] as `nn.Linear` holds them, and the X whose
        rows are the rows `rows` (or row0 .. row0+b-1) of a `csr_to_device` matrix.  Returns (loss 0-d, saved) float32 device tensors,
        `saved` = (h3 [b, hidden], logits [b, n_items], lse [b]) being what `vae_decoder_nll_bwd` takes; nothing is read back.  Range
        checks and `check` as in `csr_rows_to_dense`."""
        who = "vae_decoder_nll_fwd"
        dec, z, (b, latent, hidden, n_items), batch = self._decoder_head(who, z, w3, b3, w4, b4, csr_dev, rows, row0, b)
        h3 = torch.empty(b, hidden, dtype=torch.float32, device=self.device)
        logits = torch.empty(b, n_items, dtype=torch.float32, device=self.device)
        lse = torch.empty(b, dtype=torch.float32, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_vae_decoder_nll_fwd(self._h, C.byref(dec), _ptr(z), *batch, _ptr(h3), _ptr(logits), _ptr(lse), _ptr(loss),
                                                      _stream()), "sdrm_vae_decoder_nll_fwd")
        if check:
            self.feed_status()
        return loss, (h3, logits, lse)

    def vae_decoder_nll_bwd(self, saved, z, w3, b3, w4, b4, csr_dev, rows=None, row0=0, b=None, scale=None, need_dz=True, out=None):
        """Its backward: (dz [b, latent] | None, dw3, db3, dw4, db4) for `saved` as the forward returned it, the z and the tensors that
        forward read and the same batch.  `scale`: a float32 device tensor of one element (the upstream gradient; None = 1).
        `need_dz=False` skips the gradient of z (returned as None).  Every element of the results is written once: `out` = (dz | None,
        dw3, db3, dw4, db4) needs no zeroing.  The range checks land in the status word `feed_status` reads."""
        who = "vae_decoder_nll_bwd"
        if not isinstance(saved, (tuple, list)) or len(saved) != 3 or not all(isinstance(t, torch.Tensor) for t in saved):
            raise SdrmError(f"{who}: saved must be the (h3, logits, lse) a vae_decoder_nll_fwd returned")
        dec, z, (b, latent, hidden, n_items), batch = self._decoder_head(who, z, w3, b3, w4, b4, csr_dev, rows, row0, b)
        h3 = self._f32(who, "h3", saved[0], (b, hidden))
        logits = self._f32(who, "logits", saved[1], (b, n_items))
        lse = self._f32(who, "lse", saved[2], (b,))
        if scale is not None:
            scale = self._index(who, "scale", scale, torch.float32, 1)
        names = ("dz", "dw3", "db3", "dw4", "db4")
        shapes = ((b, latent), (hidden, latent), (hidden,), (n_items, hidden), (n_items,))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        else:
            out = tuple(None if (name == "dz" and (t is None or not need_dz)) else self._f32(who, name, t, s)
                        for name, t, s in zip(names, out, shapes))
            if need_dz and out[0] is None:
                raise SdrmError(f"{who}: out[0] (dz) is None but need_dz is set")
        dz = out[0] if need_dz else None
        self._check(self.lib.sdrm_vae_decoder_nll_bwd(self._h, C.byref(dec), _ptr(z), _ptr(h3), _ptr(logits), _ptr(lse), *batch, _ptr(scale),
                                                      _ptr(dz), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _stream()),
                    "sdrm_vae_decoder_nll_bwd")
        return (dz,) + tuple(out[1:])

    # ------------------------------------------------------------------ Adam over caller-owned tensors, the step's loss value (csrc/vae_adam.h)
    def vae_adam_step(self, params, grads, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, l2_coefs=None, l2_partials=None):
        """`torch.optim.Adam.step()` in its default form (train_SDRM.py:126, :150) for lists of float32 device tensors in ONE launch per
        16 tensors (sdrm_vae_adam_step): `params`, `exp_avg`, `exp_avg_sq` are updated in place, `grads` are read.  `step` >= 1 is the
        count after this update - the caller's number, the engine keeps nothing of the optimizer.  `l2_coefs`: per tensor the
        coefficient c of a loss term c * sum(p^2) whose gradient 2 c p is folded into the update (None: none); `l2_partials`: a
        float64 device tensor with one element per 4096-element chunk of the tensors, which then receives sum(p^2) of the weights
        before the update per chunk of every tensor with a coefficient (what `vae_loss_slot` adds up).  Returns nothing."""
        who = "vae_adam_step"
        k = len(params)
        if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == k) or (l2_coefs is not None and len(l2_coefs) != k):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: params, grads, exp_avg, exp_avg_sq (and l2_coefs) must have one entry per tensor")
        if k == 0:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_tensors <= 0")
        dev, f32 = self.device, torch.float32
        tab = (_lib.VaeAdamTensor * k)()
        for i in range(k):
            p = params[i]
            n = p.numel()
            row = tab[i]
            for name, t in (("p", p), ("g", grads[i]), ("m", exp_avg[i]), ("v", exp_avg_sq[i])):
                if not isinstance(t, torch.Tensor) or t.dtype != f32 or t.device != dev or not t.is_contiguous() or t.numel() != n:
                    raise SdrmError(f"{who}: tensor {i}: {name} must be a contiguous float32 tensor of {n} element(s) on the engine's device")
                setattr(row, name, t.data_ptr())
            row.n = n
            row.l2_coef = 0.0 if l2_coefs is None else float(l2_coefs[i])
        cap = 0
        if l2_partials is not None:
            if (not isinstance(l2_partials, torch.Tensor) or l2_partials.dtype != torch.float64 or l2_partials.device != dev
                    or not l2_partials.is_contiguous()):
                raise SdrmError(f"{who}: l2_partials must be a contiguous float64 tensor on the engine's device")
            cap = l2_partials.numel()
        self._check(self.lib.sdrm_vae_adam_step(self._h, tab, k, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                _ptr(l2_partials), cap, _stream()), "sdrm_vae_adam_step")

    def vae_loss_slot(self, neg_ll, kl, anneal, out, slot, l2_partials=None, weight_decay=0.0):
        """`out[slot] = neg_ll + anneal * kl + weight_decay * sum(l2_partials)` (train_SDRM.py:143) from two float32 device scalars, in
        torch's order of operations (sdrm_vae_loss_slot): `out` is a float32 device vector, e.g. an epoch's loss buffer, of which only
        element `slot` is written.  Without `l2_partials` the last term is +0.0, and the value is torch's to the bit.  Returns nothing."""
        who = "vae_loss_slot"
        for name, t in (("neg_ll", neg_ll), ("kl", kl)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or t.numel() != 1:
                raise SdrmError(f"{who}: {name} must be a float32 device tensor of 1 element")
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.device or out.dim() != 1 or not out.is_contiguous():
            raise SdrmError(f"{who}: out must be a contiguous float32 vector on the engine's device")
        slot = int(slot)
        if not 0 <= slot < out.numel():
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: slot {slot} outside the buffer's {out.numel()} element(s)")
        n_part = 0
        if l2_partials is not None:
            if l2_partials.dtype != torch.float64 or l2_partials.device != self.device or not l2_partials.is_contiguous():
                raise SdrmError(f"{who}: l2_partials must be a contiguous float64 tensor on the engine's device")
            n_part = l2_partials.numel()
        self._check(self.lib.sdrm_vae_loss_slot(self._h, _ptr(neg_ll), _ptr(kl), float(anneal), _ptr(l2_partials), n_part, float(weight_decay),
                                                C.c_void_p(out.data_ptr() + 4 * slot), _stream()), "sdrm_vae_loss_slot")

    def csc_to_device(self, m):
        """(colptr i64, rowidx i32, data f32 | None for an all-ones matrix, shape) of a scipy sparse matrix, on the device: the
        matrix `csr_to_device` ships (duplicates summed, indices sorted), by columns, row indices ascending within a column."""
        m = m.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        shape = m.shape
        m = m.tocsc()
        m.sort_indices()
        data = None if np.all(m.data == 1) else torch.from_numpy(m.data.astype(np.float32)).to(self.device)
        return (torch.from_numpy(m.indptr.astype(np.int64)).to(self.device),
                torch.from_numpy(m.indices.astype(np.int32)).to(self.device), data, shape)

    def csr_to_device(self, m):
        """(indptr i64, indices i32, data f32 | None for an all-ones matrix, shape) of a scipy sparse matrix, on the device."""
        m = m.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        data = None if np.all(m.data == 1) else torch.from_numpy(m.data.astype(np.float32)).to(self.device)
        return (torch.from_numpy(m.indptr.astype(np.int64)).to(self.device),
                torch.from_numpy(m.indices.astype(np.int32)).to(self.device), data, m.shape)

    CSR_STACK_MAX = 8          # parts of one csr_vstack
    CSR_TRANSPOSE_WORDS = 2 ** 26   # most words of csr_transpose's bit table, ceil(n_rows / 64) x n_cols

    def _csr_arrays(self, who, name, csr_dev):
        """(indptr, indices, data | None, n_rows, n_cols, capacity) of a device CSR tuple, checked on the host: the 4-tuple of
        `csr_to_device` / `holdout_split` or the 3-tuple (indptr, indices, shape) of `equal_sparsity_csr`.  `capacity` is the size of
        the index array; the entry count lives in indptr."""
        if not isinstance(csr_dev, tuple) or len(csr_dev) not in (3, 4):
            raise SdrmError(f"{who}: {name} must be a device CSR tuple (indptr, indices, data | None, shape) or (indptr, indices, shape)")
        indptr, indices, data, shape = csr_dev if len(csr_dev) == 4 else (csr_dev[0], csr_dev[1], None, csr_dev[2])
        n_rows, n_cols = int(shape[0]), int(shape[1])
        indptr = self._index(who, f"{name} indptr", indptr, torch.int64, n_rows + 1)
        if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32 or indices.device != self.device or not indices.is_contiguous():
            raise SdrmError(f"{who}: {name} indices must be a contiguous int32 tensor on the engine's device")
        capacity = int(indices.numel())
        if data is not None:
            data = self._f32(who, f"{name} data", data, (capacity,))
        return indptr, indices, data, n_rows, n_cols, capacity

    def csr_transpose(self, csr_dev, check=True, out=None):
        """The CSC form of a device CSR matrix (sdrm_csr_transpose, csrc/csr_transpose.h), shaped like `csc_to_device`'s result:
        (colptr int64 [n_cols + 1], rowidx int32, data float32 | None, shape).  Row indices ascend within a column; for a canonical
        input these are the bytes `csc_to_device` ships.  The columns of a row must be distinct and need not be sorted; indptr may
        hold absolute offsets into longer arrays (a row range of a larger matrix: slice its indptr and say the rows in the shape).
        `rowidx` and `data` have the input's capacity and are filled up to colptr[-1].  Nothing is read back; range checks and
        `check` as in `csr_rows_to_dense`, and a row that holds a column twice is reported there too.  `out`: (colptr, rowidx,
        data | None) device tensors to fill.  Refused (SDRM_ERR_SHAPE) beyond 2^22 rows or columns or a bit table of
        ceil(n_rows / 64) x n_cols > 2^26 words: `csc_to_device` takes such a matrix on the host."""
        who = "csr_transpose"
        indptr, indices, data, n_rows, n_cols, capacity = self._csr_arrays(who, "csr", csr_dev)
        if not (1 <= n_rows <= 2 ** 22 and 1 <= n_cols <= 2 ** 22) or -(-n_rows // 64) * n_cols > self.CSR_TRANSPOSE_WORDS:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {n_rows} x {n_cols} is outside 1 .. 2^22 rows and columns or needs a bit table above 2^26 words")
        if out is None:
            out = (torch.empty(n_cols + 1, dtype=torch.int64, device=self.device), torch.empty(capacity, dtype=torch.int32, device=self.device),
                   None if data is None else torch.empty(capacity, dtype=torch.float32, device=self.device))
        colptr = self._index(who, "out colptr", out[0], torch.int64, n_cols + 1)
        rowidx = self._index(who, "out rowidx", out[1], torch.int32, capacity)
        if (data is None) != (out[2] is None):
            raise SdrmError(f"{who}: SDRM_ERR_ARG: out carries values exactly when the input does")
        cdata = None if data is None else self._f32(who, "out data", out[2], (capacity,))
        # a matrix without an entry: torch gives an empty tensor no address, and the C ABI takes no null array
        spare = (indices, rowidx, data, cdata) if capacity else (indices.new_zeros(1), indices.new_zeros(1)) + ((None, None) if data is None else (
            torch.zeros(1, dtype=torch.float32, device=self.device), torch.zeros(1, dtype=torch.float32, device=self.device)))
        self._check(self.lib.sdrm_csr_transpose(self._h, _ptr(indptr), _ptr(spare[0]), _ptr(spare[2]), n_rows, n_cols, capacity, _ptr(colptr),
                                                _ptr(spare[1]), _ptr(spare[3]), _stream()), "sdrm_csr_transpose")
        self._feed_keep = spare
        if check:
            self.feed_status()
        return colptr, rowidx, cdata, (n_rows, n_cols)

    def csr_vstack(self, parts, check=True):
        """`scipy.sparse.vstack` of up to 8 device CSR matrices of one width (sdrm_csr_vstack, csrc/csr_transpose.h): a list of
        `csr_to_device`-shaped tuples - `holdout_split`'s outputs as they are, whose arrays are longer than their entry counts - or
        3-tuples of `equal_sparsity_csr`.  Returns a `csr_to_device`-shaped tuple: indptr from 0, the rows in part order with their
        entries in their own order, `data` None when no part has values (else float32, an all-ones part contributing 1.0).  The index
        array has the sum of the parts' capacities and is filled up to indptr[-1]; nothing is read back.  A row with a bad indptr pair
        or a column outside the width is EMPTY in the output and raises the feed status word (`check` as in `csr_rows_to_dense`)."""
        who = "csr_vstack"
        parts = list(parts)
        if not 1 <= len(parts) <= self.CSR_STACK_MAX:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {len(parts)} parts, outside 1 .. {self.CSR_STACK_MAX}")
        arrays = [self._csr_arrays(who, f"part {i}", p) for i, p in enumerate(parts)]
        n_cols = arrays[0][4]
        if any(a[4] != n_cols for a in arrays):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: the parts have {[a[4] for a in arrays]} columns, not one width")
        rows, capacity = sum(a[3] for a in arrays), sum(a[5] for a in arrays)
        if not (1 <= rows <= 2 ** 22 and 1 <= n_cols <= 2 ** 22):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {rows} rows x {n_cols} columns, outside 1 .. 2^22")
        values = any(a[2] is not None and a[5] > 0 for a in arrays)   # (an empty array has no address: such a part has no values to give)
        indptr = torch.empty(rows + 1, dtype=torch.int64, device=self.device)
        indices = torch.empty(capacity, dtype=torch.int32, device=self.device)
        data = torch.empty(capacity, dtype=torch.float32, device=self.device) if values else None
        spare = indices.new_zeros(1)   # a part without an entry: torch gives an empty tensor no address, and the C ABI takes no null array
        desc = (_lib.CsrPart * len(arrays))()
        for d, (ip, ix, dv, n_rows, _, cap) in zip(desc, arrays):
            d.indptr, d.indices, d.data = ip.data_ptr(), (ix if cap else spare).data_ptr(), dv.data_ptr() if dv is not None and cap else None
            d.n_rows, d.capacity = n_rows, cap
        self._check(self.lib.sdrm_csr_vstack(self._h, desc, len(arrays), n_cols, _ptr(indptr), _ptr(indices if capacity else spare), _ptr(data), capacity,
                                             _stream()), "sdrm_csr_vstack")
        self._feed_keep = (spare, arrays)
        if check:
            self.feed_status()
        return indptr, indices, data, (rows, n_cols)

    def csr_rows_to_dense(self, csr_dev, rows=None, row0=0, b=None, check=True):
        """dataloaders.py:46-79 + `.to_dense()` (train_SDRM.py:323) on the device: dense float32 [b, n_items] of the rows
        `rows` (int64 tensor, e.g. a slice of the epoch permutation) or row0 .. row0+b-1 of a `csr_to_device` matrix.
        Row ids and column indices are range-checked ON THE DEVICE (an offending row / entry stays zero, never a stray store);
        `check=True` reads the verdict back at once (one stream sync) and raises, `check=False` leaves it to a later
        `feed_status()` - what an epoch loop wants (`pipeline.DeviceFeed` asks once per epoch)."""
        _, n_items, b, batch = self._csr_batch("csr_rows_to_dense", csr_dev, rows, row0, b)
        out = torch.empty(b, n_items, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_csr_rows_to_dense(self._h, *batch, n_items, _ptr(out), _stream()), "sdrm_csr_rows_to_dense")
        if check:
            self.feed_status()
        return out

    def feed_status(self):
        """Raises if any launch on the CSR feed since the last call met a row id, column index or indptr pair outside the matrix."""
        self._check(self.lib.sdrm_feed_status(self._h, _stream()), "sdrm_feed_status")

    def holdout_split(self, csr_dev, test_prop=0.2, seed=0, draw=0, check=True, out=None):
        """utilities.py:174-236 on the device (sdrm_holdout_split, csrc/holdout.h): the per-user hold-out split of a `csr_to_device`
        matrix as (train_csr_dev, held_csr_dev), each an `(indptr, indices, None, shape)` tuple like `csr_to_device`'s - all ones,
        the input's row numbering, users with fewer than two entries as empty rows in both.  Per user with n >= 2 entries,
        ceil(test_prop * n) go to the held part, chosen by the engine's Philox keys of (seed, draw, row, place) - not numpy's
        generator.  The index tensors have the input's nnz as capacity and are filled up to indptr[-1].  Nothing is read back;
        range checks and `check` as in `csr_rows_to_dense`.  `out`: a pair of int32 device tensors of nnz elements to fill."""
        who = "holdout_split"
        indptr, indices, _, (n_rows, n_items) = csr_dev
        n_rows, n_items, nnz = int(n_rows), int(n_items), int(indices.numel())
        indptr = self._index(who, "indptr", indptr, torch.int64, n_rows + 1)
        indices = self._index(who, "indices", indices, torch.int32, nnz)
        if out is None:
            out = (torch.empty(nnz, dtype=torch.int32, device=self.device), torch.empty(nnz, dtype=torch.int32, device=self.device))
        tr_idx, he_idx = (self._index(who, "out", t, torch.int32, nnz) for t in out)
        tr_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        he_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        # a matrix without an entry: torch gives an empty tensor no address, and the C ABI takes no null array
        spare = [indices.new_zeros(1) for _ in range(3)] if nnz == 0 else (indices, tr_idx, he_idx)
        self._check(self.lib.sdrm_holdout_split(self._h, _ptr(indptr), _ptr(spare[0]), n_rows, n_items, nnz, float(test_prop),
                                                int(seed) & (2 ** 64 - 1), int(draw) & 0xFFFFFFFF, _ptr(tr_ptr), _ptr(spare[1]),
                                                _ptr(he_ptr), _ptr(spare[2]), _stream()), "sdrm_holdout_split")
        if check:
            self.feed_status()
        return (tr_ptr, tr_idx, None, (n_rows, n_items)), (he_ptr, he_idx, None, (n_rows, n_items))

    def _rank_tables(self, ks):
        """(ks int32 host array, tp, idcg float64 device tables) of a cut-off list, made once per list and engine."""
        key = tuple(int(k) for k in ks)
        hit = self._rank_cache.get(key)
        if hit is None:
            ks_h = np.asarray(key, dtype=np.int32)
            kmax = int(ks_h.max())
            tp = 1.0 / np.log2(np.arange(2, kmax + 2))                                   # utilities.py:145
            idcg = np.asarray([tp[:m].sum() for m in range(kmax + 1)], dtype=np.float64)   # utilities.py:149-150
            hit = self._rank_cache[key] = (ks_h, torch.from_numpy(tp).to(self.device), torch.from_numpy(idcg).to(self.device))
        return hit

    def rank_metrics(self, scores, heldout, train=None, ks=(1, 3, 5, 10, 20, 50), row0=0):
        """utilities.py:116-171 on the device: (recall[nk,U], ndcg[nk,U]) float64 device tensors for a score matrix
        [U, I] (device or host) against the held-out CSR matrix, with the items of the `train` CSR matrix masked out
        (-inf).  `heldout` / `train` are scipy.sparse matrices (or anything with tocsr()) of the scores' shape - or device CSR
        tuples (`csr_to_device`, `holdout_split`) of [n_rows, I]: the batch's U rows are then rows row0 .. row0+U-1 of them, the
        discount tables come from a per-`ks` cache on the engine, and the call uploads nothing.  The device form trusts its column
        indices (`holdout_split` delivers checked ones)."""
        scores = self._dev(scores, torch.float32)
        U, I = scores.shape
        if isinstance(heldout, tuple):
            return self._rank_metrics_dev(scores, heldout, train, ks, int(row0))
        if isinstance(train, tuple):
            raise SdrmError("rank_metrics: heldout and train must both be scipy matrices or both device CSR tuples")
        if row0:
            raise SdrmError("rank_metrics: row0 goes with device CSR tuples only")
        ks = np.asarray(ks, dtype=np.int32)
        kmax = int(ks.max())
        tp = 1.0 / np.log2(np.arange(2, kmax + 2))                                   # utilities.py:145
        idcg = np.asarray([tp[:m].sum() for m in range(kmax + 1)], dtype=np.float64)   # utilities.py:149-150

        def csr(m):
            m = m.tocsr()
            if m.shape != (U, I):
                raise SdrmError(f"rank_metrics: sparse matrix shape {m.shape} != scores shape {(U, I)}")
            return (torch.from_numpy(m.indptr.astype(np.int64)).to(self.device),
                    torch.from_numpy(m.indices.astype(np.int32)).to(self.device))
        hp, hi = csr(heldout)
        tr = csr(train) if train is not None else (None, None)
        tp_d, idcg_d = torch.from_numpy(tp).to(self.device), torch.from_numpy(idcg).to(self.device)
        recall = torch.empty(len(ks), U, dtype=torch.float64, device=self.device)
        ndcg = torch.empty(len(ks), U, dtype=torch.float64, device=self.device)
        self._check(self.lib.sdrm_rank_metrics(self._h, _ptr(scores), U, I, _ptr(hp), _ptr(hi), _ptr(tr[0]), _ptr(tr[1]),
                                               ks.ctypes.data_as(C.c_void_p), len(ks), _ptr(tp_d), _ptr(idcg_d),
                                               _ptr(recall), _ptr(ndcg), _stream()), "sdrm_rank_metrics")
        self._keepalive = (scores, hp, hi, tr, tp_d, idcg_d)
        return recall, ndcg

    def _rank_metrics_dev(self, scores, heldout, train, ks, row0):
        U, I = scores.shape
        if train is not None and not isinstance(train, tuple):
            raise SdrmError("rank_metrics: heldout and train must both be scipy matrices or both device CSR tuples")

        def rows(name, csr_dev):
            indptr, indices, _, (n_rows, width) = csr_dev
            if int(width) != I:
                raise SdrmError(f"rank_metrics: SDRM_ERR_SHAPE: the {name} matrix has {width} columns, the scores {I}")
            if row0 < 0 or row0 + U > int(n_rows):
                raise SdrmError(f"rank_metrics: SDRM_ERR_SHAPE: rows {row0} .. {row0 + U - 1} end behind the {name} matrix's {n_rows} rows")
            indptr = self._index("rank_metrics", f"{name} indptr", indptr, torch.int64, int(n_rows) + 1)
            if indices.dtype != torch.int32 or indices.device != self.device or not indices.is_contiguous():
                raise SdrmError(f"rank_metrics: {name} indices must be a contiguous int32 tensor on the engine's device")
            if indices.numel() == 0:
                indices = indices.new_zeros(1)
            return indptr[row0:], indices   # indptr holds absolute offsets: a row range is a pointer offset
        hp, hi = rows("held-out", heldout)
        tr = rows("train", train) if train is not None else (None, None)
        ks_h, tp_d, idcg_d = self._rank_tables(ks)
        recall = torch.empty(len(ks_h), U, dtype=torch.float64, device=self.device)
        ndcg = torch.empty(len(ks_h), U, dtype=torch.float64, device=self.device)
        self._check(self.lib.sdrm_rank_metrics(self._h, _ptr(scores), U, I, _ptr(hp), _ptr(hi), _ptr(tr[0]), _ptr(tr[1]),
                                               ks_h.ctypes.data_as(C.c_void_p), len(ks_h), _ptr(tp_d), _ptr(idcg_d),
                                               _ptr(recall), _ptr(ndcg), _stream()), "sdrm_rank_metrics")
        self._keepalive = (scores, hp, hi, tr)
        return recall, ndcg

    # ------------------------------------------------------------------ truncated-SVD evaluator (csrc/svd_eval.h)
    SVD_PANEL = 32   # columns of the fit's panel: n_components + the reference's 10 oversampling columns must fit

    def _sparse_dev(self, who, name, sp_dev):
        """(indptr, indices, data, n_rows, n_cols, nnz) of a `csr_to_device` / `csc_to_device` tuple, checked; an empty index array is
        replaced by one element (torch gives an empty tensor no address, and the C ABI takes no null array)."""
        indptr, indices, data, (n_rows, n_cols) = sp_dev
        n_rows, n_cols, nnz = int(n_rows), int(n_cols), int(indices.numel())
        major = n_cols if name == "csc" else n_rows
        indptr = self._index(who, f"{name} indptr", indptr, torch.int64, major + 1)
        indices = self._index(who, f"{name} indices", indices, torch.int32, nnz)
        if data is not None:
            data = self._f32(who, f"{name} data", data, (nnz,))
        if nnz == 0:
            indices = indices.new_zeros(1)
        return indptr, indices, data, n_rows, n_cols, nnz

    def svd_fit(self, csr_dev, csc_dev, n_components=20, n_iter=100, seed=0, draw=0, q0=None):
        """`TruncatedSVD(n_components, n_iter=n_iter).fit` (svd_benchmark.py:47-48) on the device, sdrm_svd_fit: the subspace iteration of
        sklearn's randomized SVD on a panel of 32 columns, from the `csr_to_device` and `csc_to_device` tuples of ONE matrix [m, n].
        Returns (components [n_components, n] float32 device tensor, singular_values [n_components] float64 numpy array, descending).
        The start panel is drawn on the device from Philox keys of (seed, draw), or is `q0` [n, 32] (float32, host or device).  The
        sign of a component is the iteration's own.  Refused with SDRM_ERR_SHAPE before anything is launched: n_components < 1,
        n_components + 10 > 32, min(m, n) < 32.  A matrix of numerical rank below 32 breaks the panel's factorisation down: the call
        raises (SDRM_ERR_ARG), and the next fit on this engine works.  The call synchronises (one read-back) and asks `feed_status()`."""
        who = "svd_fit"
        k, n_iter = int(n_components), int(n_iter)
        indptr, indices, data, m, n, nnz = self._sparse_dev(who, "csr", csr_dev)
        colptr, rowidx, cdata, m2, n2, nnz2 = self._sparse_dev(who, "csc", csc_dev)
        if (m2, n2, nnz2) != (m, n, nnz) or (data is None) != (cdata is None):
            raise SdrmError(f"{who}: SDRM_ERR_ARG: the CSR form is {(m, n)} with {nnz} entries, the CSC form {(m2, n2)} with {nnz2}: not one matrix")
        if k < 1 or k + 10 > self.SVD_PANEL or min(m, n) < self.SVD_PANEL or n_iter < 0:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_components = {k} outside 1 .. {self.SVD_PANEL - 10}, min(m, n) = {min(m, n)} < {self.SVD_PANEL} "
                            f"or n_iter = {n_iter} < 0")
        if q0 is not None:
            q0 = self._f32(who, "q0", self._dev(q0, torch.float32), (n, self.SVD_PANEL))
        components = torch.empty(k, n, dtype=torch.float32, device=self.device)
        sigma = np.zeros(k, dtype=np.float64)
        self._check(self.lib.sdrm_svd_fit(self._h, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(colptr), _ptr(rowidx), _ptr(cdata), m, n, nnz, k,
                                          n_iter, int(seed) & (2 ** 64 - 1), int(draw) & 0xFFFFFFFF, _ptr(q0), _ptr(components),
                                          sigma.ctypes.data_as(C.c_void_p), _stream()), "sdrm_svd_fit")
        self.feed_status()
        return components, sigma

    def svd_scores(self, csr_dev, components, rows=None, row0=0, b=None, check=True):
        """`svd.inverse_transform(svd.transform(X))` (svd_benchmark.py:48-49) for a batch of rows of a `csr_to_device` matrix, sdrm_svd_scores:
        the dense float32 [b, n_items] device tensor (X_rows V^T) V that `rank_metrics` takes, V = `components` [k, n_items] as `svd_fit`
        returns them.  `rows` (int64) or row0 .. row0+b-1.  Seen items are not masked here.  Range checks and `check` as in
        `csr_rows_to_dense`: a row or entry that fails contributes zeros."""
        who = "svd_scores"
        n_rows, n_items, b, batch = self._csr_batch(who, csr_dev, rows, row0, b)
        if not isinstance(components, torch.Tensor) or components.dim() != 2:
            raise SdrmError(f"{who}: components must be a 2-D float32 tensor [k, n_items]")
        k = int(components.shape[0])
        components = self._f32(who, "components", components, (k, n_items))
        if not 1 <= k <= self.SVD_PANEL - 10:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {k} components outside 1 .. {self.SVD_PANEL - 10}")
        indptr, indices, data, n_rows_, row_ids, row0_, b_ = batch
        nnz = int(csr_dev[1].numel())
        out = torch.empty(b, n_items, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_svd_scores(self._h, indptr, indices, data, n_rows_, nnz, row_ids, row0_, b_, n_items, _ptr(components), k,
                                             _ptr(out), _stream()), "sdrm_svd_scores")
        if check:
            self.feed_status()
        return out

    def debug_svd_stage(self, sp_dev, q, transposed=False):
        """One product and one orthonormalisation of the fit on a caller's panel (sdrm_debug_svd_stage): (A q, orth(A q)) as float32 device
        tensors [rows, 32] for a `csr_to_device` tuple, or (A^T q, orth(A^T q)) for a `csc_to_device` tuple with `transposed=True`."""
        who = "debug_svd_stage"
        indptr, indices, data, m, n, nnz = self._sparse_dev(who, "csc" if transposed else "csr", sp_dev)
        rows, cols = (n, m) if transposed else (m, n)
        q = self._f32(who, "q", self._dev(q, torch.float32), (cols, self.SVD_PANEL))
        y = torch.empty(rows, self.SVD_PANEL, dtype=torch.float32, device=self.device)
        y_orth = torch.empty_like(y)
        self._check(self.lib.sdrm_debug_svd_stage(self._h, _ptr(indptr), _ptr(indices), _ptr(data), rows, cols, nnz, _ptr(q), _ptr(y), _ptr(y_orth),
                                                  _stream()), "sdrm_debug_svd_stage")
        self.feed_status()
        return y, y_orth

    # ------------------------------------------------------------------ NMF evaluator (csrc/nmf.h)
    NMF_LD = 16      # row stride of a factor in the C ABI, and the most components

    def _nmf_factor(self, who, name, a, rows, k):
        """A factor [rows, k] (host or device) as the C ABI stores it: float64 [rows, 16] on the device, columns k .. 15 zero."""
        t = self._dev(a, torch.float64)
        if tuple(t.shape) != (rows, k):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {name} must be {[rows, k]}, got {list(t.shape)}")
        out = torch.zeros(rows, self.NMF_LD, dtype=torch.float64, device=self.device)
        out[:, :k] = t
        return out

    def _nmf_init(self, who, csr, m, n, nnz, k, csr_dev, csc_dev, seed, draw, svd_iter):
        """(W0 [m, 16], Ht0 [n, 16]) as sdrm_nmf_init leaves them, from svd_fit's factors."""
        if svd_iter is None:
            svd_iter = 7 if k < 0.1 * min(m, n) else 4     # sklearn's n_iter='auto'
        components, sigma = self.svd_fit(csr_dev, csc_dev, n_components=k, n_iter=int(svd_iter), seed=seed, draw=draw)
        w0 = torch.zeros(m, self.NMF_LD, dtype=torch.float64, device=self.device)
        ht0 = torch.zeros(n, self.NMF_LD, dtype=torch.float64, device=self.device)
        indptr, indices, data = csr
        self._check(self.lib.sdrm_nmf_init(self._h, _ptr(indptr), _ptr(indices), _ptr(data), m, n, nnz, k, _ptr(components),
                                           sigma.ctypes.data_as(C.c_void_p), _ptr(w0), _ptr(ht0), _stream()), "sdrm_nmf_init")
        return w0, ht0

    def nmf_init(self, csr_dev, csc_dev, n_components=15, seed=0, draw=0, svd_iter=None):
        """sklearn's `_initialize_nmf(X, n_components, init='nndsvda')` - NMF's default start - on the device, sdrm_nmf_init, with
        `svd_fit(csr_dev, csc_dev, n_components, n_iter=svd_iter, seed, draw)` in the place of sklearn's randomized SVD (`svd_iter=None`
        follows its 'auto' rule: 7 iterations when n_components < 0.1 min(m, n), else 4).  Returns (W0 [m, k], H0 [k, n]) float64 device
        tensors, every entry positive.  It inherits `svd_fit`'s refusals: n_components + 10 > 32, min(m, n) < 32, a matrix of numerical
        rank below 32.  The call synchronises (svd_fit's read-back) and asks `feed_status()`."""
        who = "nmf_init"
        k = int(n_components)
        indptr, indices, data, m, n, nnz = self._sparse_dev(who, "csr", csr_dev)
        if not 1 <= k <= self.NMF_LD:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_components = {k} outside 1 .. {self.NMF_LD}")
        w0, ht0 = self._nmf_init(who, (indptr, indices, data), m, n, nnz, k, csr_dev, csc_dev, seed, draw, svd_iter)
        self.feed_status()
        return w0[:, :k].contiguous(), ht0[:, :k].t().contiguous()

    def nmf_fit(self, csr_dev, csc_dev, n_components=15, max_iter=50, tol=1e-4, init=None, seed=0, check=True):
        """`NMF(n_components, max_iter=max_iter, tol=tol).fit` (svd_benchmark.py:50-53; sklearn's `cd` solver without regularisation or
        shuffle) on the device, sdrm_nmf_fit, from the `csr_to_device` and `csc_to_device` tuples of ONE matrix [m, n].  `init=(W0
        [m, k], H0 [k, n])` (host or device) is sklearn's init='custom'; otherwise the start is `nmf_init(..., seed=seed)`.  Returns
        (W [m, k], H [k, n] float64 device tensors, n_iter, violations float64 numpy array [n_iter]): the iterations run, and the
        violation v_i of each (the fit stops when v_i / v_1 <= tol).  The whole fit is queued without a host round trip; the call then
        reads n_iter and the violations back in one copy and, with `check`, asks `feed_status()`.  The same bits on every call."""
        who = "nmf_fit"
        k, max_iter, tol = int(n_components), int(max_iter), float(tol)
        indptr, indices, data, m, n, nnz = self._sparse_dev(who, "csr", csr_dev)
        colptr, rowidx, cdata, m2, n2, nnz2 = self._sparse_dev(who, "csc", csc_dev)
        if (m2, n2, nnz2) != (m, n, nnz) or (data is None) != (cdata is None):
            raise SdrmError(f"{who}: SDRM_ERR_ARG: the CSR form is {(m, n)} with {nnz} entries, the CSC form {(m2, n2)} with {nnz2}: not one matrix")
        if not 1 <= k <= self.NMF_LD or not 1 <= max_iter <= 10000 or not tol >= 0:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_components = {k} outside 1 .. {self.NMF_LD}, max_iter = {max_iter} outside 1 .. 10000 or tol = {tol} < 0")
        if init is None:
            w, ht = self._nmf_init(who, (indptr, indices, data), m, n, nnz, k, csr_dev, csc_dev, seed, 0, None)
        else:
            w = self._nmf_factor(who, "W0", init[0], m, k)
            ht = self._nmf_factor(who, "H0^T", self._dev(init[1], torch.float64).t(), n, k)
        tail = torch.zeros(max_iter + 1, dtype=torch.float64, device=self.device)   # violations [max_iter] | n_iter (int32) in the last slot
        n_iter_ptr = C.c_void_p(tail.data_ptr() + 8 * max_iter)
        self._check(self.lib.sdrm_nmf_fit(self._h, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(colptr), _ptr(rowidx), _ptr(cdata), m, n, nnz, k,
                                          max_iter, tol, _ptr(w), _ptr(ht), n_iter_ptr, _ptr(tail), _stream()), "sdrm_nmf_fit")
        host = tail.cpu().numpy()
        n_iter = int(host[max_iter:].view(np.int32)[0])
        if check:
            self.feed_status()
        return w[:, :k].contiguous(), ht[:, :k].t().contiguous(), n_iter, host[:n_iter].copy()

    def nmf_scores(self, W, H, rows=None, row0=0, b=None, check=True):
        """`nmf.inverse_transform(W)` (svd_benchmark.py:54) for a batch of rows of W, sdrm_nmf_scores: the dense float32 [b, n_items]
        device tensor W[rows] H that `rank_metrics` takes, every element added in float64 and rounded once.  W [m, k], H [k, n_items]
        as `nmf_fit` returns them (host or device); `rows` (int64) or row0 .. row0+b-1 (all rows when neither is given).  Seen items
        are not masked here.  A row id outside W gives a zero row and raises the feed status word (`check` as in `csr_rows_to_dense`)."""
        who = "nmf_scores"
        if W.ndim != 2 or H.ndim != 2 or W.shape[1] != H.shape[0]:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: W must be [m, k] and H [k, n_items]")
        m, k, n_items = int(W.shape[0]), int(W.shape[1]), int(H.shape[1])
        if not 1 <= k <= self.NMF_LD:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {k} components outside 1 .. {self.NMF_LD}")
        w = self._nmf_factor(who, "W", W, m, k)
        ht = self._nmf_factor(who, "H^T", self._dev(H, torch.float64).t(), n_items, k)
        if rows is not None:
            rows = self._dev(rows, torch.int64)
            b = rows.numel()
        elif b is None:
            row0, b = 0, m
        row0, b = int(row0), int(b)
        if b < 1 or row0 < 0 or (rows is None and row0 + b > m):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: rows {row0} .. {row0 + b - 1} end behind W's {m} rows, or there is none")
        out = torch.empty(b, n_items, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_nmf_scores(self._h, _ptr(w), _ptr(ht), m, k, _ptr(rows), row0, b, n_items, _ptr(out), _stream()), "sdrm_nmf_scores")
        self._feed_keep = (rows, w, ht)
        if check:
            self.feed_status()
        return out

    # ------------------------------------------------------------------ NeuMF evaluator's forward (csrc/neumf.h)
    NEUMF_FACTORS = (8, 16, 32)
    NEUMF_TENSORS = ("embed_user_GMF.weight", "embed_item_GMF.weight", "embed_user_MLP.weight", "embed_item_MLP.weight", "MLP_layers.1.weight",
                     "MLP_layers.1.bias", "MLP_layers.4.weight", "MLP_layers.4.bias", "MLP_layers.7.weight", "MLP_layers.7.bias",
                     "predict_layer.weight", "predict_layer.bias")

    def _neumf(self, who, weights):
        """The twelve tensors of a live NeuMF-end module with three MLP layers, in `NEUMF_TENSORS` (= `state_dict`) order, checked on the host
        and handed on as they are: (sdrm_neumf struct, n_users, n_items, factor).  Refused: anything but twelve tensors (a tower of another
        depth), a factor outside `NEUMF_FACTORS`, a tensor of another dtype / device / shape, tables whose row counts disagree."""
        weights = list(weights.values()) if isinstance(weights, dict) else list(weights)
        if len(weights) != len(self.NEUMF_TENSORS):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {len(weights)} tensors; NeuMF-end with THREE MLP layers has twelve ({', '.join(self.NEUMF_TENSORS)})")
        pg = weights[0]
        if not isinstance(pg, torch.Tensor) or pg.dim() != 2:
            raise SdrmError(f"{who}: {self.NEUMF_TENSORS[0]} must be a 2-D float32 tensor [n_users, factor]")
        n_users, F = int(pg.shape[0]), int(pg.shape[1])
        if F not in self.NEUMF_FACTORS:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: factor {F} outside {self.NEUMF_FACTORS}")
        n_items = int(weights[1].shape[0]) if isinstance(weights[1], torch.Tensor) and weights[1].dim() == 2 else -1
        if n_users < 1 or n_items < 1:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: a table without rows")
        shapes = ((n_users, F), (n_items, F), (n_users, 4 * F), (n_items, 4 * F), (4 * F, 8 * F), (4 * F,), (2 * F, 4 * F), (2 * F,), (F, 2 * F), (F,),
                  (1, 2 * F), (1,))
        ts = [self._f32(who, name, t.detach() if isinstance(t, torch.Tensor) else t, shape) for name, t, shape in zip(self.NEUMF_TENSORS, weights, shapes)]
        return _lib.Neumf(*[t.data_ptr() for t in ts], n_users, n_items, F), ts, n_users, n_items

    def _ids(self, who, name, ids):
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or ids.device != self.device or not ids.is_contiguous():
            raise SdrmError(f"{who}: {name} must be a contiguous 1-D int32 tensor on the engine's device")
        if ids.numel() < 1:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {name} is empty")
        return ids

    def neumf_scores(self, weights, users, items=None, out=None, check=True):
        """neural_cf_benchmark_pt.py:219-233 / :299-310 on the device (sdrm_neumf_scores): the eval-mode logits of every listed user against
        every listed item, dense float32 [len(users), len(items)] as `rank_metrics` takes it.  `weights`: the live module's twelve float32
        tensors (`NEUMF_TENSORS` order, e.g. `list(model.state_dict().values())`), read in place.  `users`: int32 device tensor, any order,
        repeats allowed; `items`: the same, or None for 0 .. n_items - 1.  Ids are range-checked on the device (an offending row / column is
        zero); `check` as in `csr_rows_to_dense`."""
        who = "neumf_scores"
        w, keep, n_users, n_items = self._neumf(who, weights)
        users = self._ids(who, "users", users)
        if items is not None:
            items = self._ids(who, "items", items)
        nu, ni = users.numel(), n_items if items is None else items.numel()
        if nu > 2 ** 20 - 16 or ni > 2 ** 22 or nu * ni >= 2 ** 40:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {nu} users x {ni} items: more than 2^20 - 16 users, 2^22 items or 2^40 - 1 pairs")
        if out is None:
            out = torch.empty(nu, ni, dtype=torch.float32, device=self.device)
        out = self._f32(who, "out", out, (nu, ni))
        self._check(self.lib.sdrm_neumf_scores(self._h, C.byref(w), _ptr(users), nu, _ptr(items), ni, _ptr(out), _stream()), "sdrm_neumf_scores")
        if check:
            self.feed_status()
        return out

    def neumf_pair_logits(self, weights, users, items, labels=None, check=True):
        """neural_cf_benchmark_pt.py:209-210 on the device (sdrm_neumf_pair_loss): (logits [n] float32, loss_sum) for the listed pairs
        (users[j], items[j]), int32 device tensors of one length.  With `labels` (float32 device tensor [n]) loss_sum is a device float64
        scalar tensor, the sum of BCEWithLogitsLoss's terms in a fixed order (divide by n for the loss); without, None.  A pair with an id
        outside its table has logit 0 and adds nothing to the sum."""
        who = "neumf_pair_logits"
        w, keep, n_users, n_items = self._neumf(who, weights)
        users, items = self._ids(who, "users", users), self._ids(who, "items", items)
        n = users.numel()
        if items.numel() != n:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {n} users against {items.numel()} items")
        loss_sum = None
        if labels is not None:
            labels = self._f32(who, "labels", labels, (n,))
            loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        logits = torch.empty(n, dtype=torch.float32, device=self.device)
        self._check(self.lib.sdrm_neumf_pair_loss(self._h, C.byref(w), _ptr(users), _ptr(items), _ptr(labels), n, _ptr(logits), _ptr(loss_sum),
                                                  _stream()), "sdrm_neumf_pair_loss")
        if check:
            self.feed_status()
        return logits, loss_sum

    # ------------------------------------------------------------------ NeuMF evaluator's train steps (csrc/neumf_train.h)
    NEUMF_TRAIN_FACTORS = (8, 16)
    NEUMF_TRAIN_MAX_BATCH = 1024

    def neumf_train_steps(self, weights, exp_avg, exp_avg_sq, triples, batch, step0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, p_drop=0.5, seed=0,
                          call_id=0, keep=None, grads=None, check=True):
        """neural_cf_benchmark_pt.py:186-200 on the device (sdrm_neumf_train_steps): ceil(n / batch) consecutive train steps of NeuMF-end
        over `triples` (int32 device tensor [n, 3]: user, item, label) in order, the last batch partial - train-mode forward with the
        three dropouts, BCEWithLogitsLoss, the gradients of all twelve tensors and `torch.optim.Adam`'s dense update, all enqueued by this
        one call with no host synchronisation between steps.  `weights`: the live module's twelve float32 tensors (`NEUMF_TENSORS` order),
        UPDATED IN PLACE; `exp_avg`, `exp_avg_sq`: twelve tensors of the same shapes, Adam's moments, updated in place.  Adam's step count
        for step t of the call is `step0 + t + 1` - the caller's number, the engine keeps nothing of the optimizer.
        Dropout: with `keep` (uint8 device tensor [n, 14 factor]; per pair 8 factor bytes for the input of layer 1, 4 factor for layer 2,
        2 factor for layer 3, non-zero = kept) the masks are the caller's; without, they are Philox4x32-10's of (seed, call_id, the pair's
        place in `triples`, column) - never torch's generator.  `grads`: twelve float32 tensors of the weights' shapes that receive the
        dense gradients of the LAST step.  Ids are range-checked on the device (such a pair adds nothing, the divisor still counts it);
        `check` as in `csr_rows_to_dense`.  Returns the per-step losses, a float64 device tensor [ceil(n / batch)]."""
        who = "neumf_train_steps"
        w, ts, n_users, n_items = self._neumf(who, weights)
        F = int(ts[0].shape[1])
        if F not in self.NEUMF_TRAIN_FACTORS:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: factor {F} outside {self.NEUMF_TRAIN_FACTORS} (the train step is not built for 32)")
        lists = {"exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
        if grads is not None:
            lists["grads"] = grads
        checked = {}
        for lname, lst in lists.items():
            lst = list(lst.values()) if isinstance(lst, dict) else list(lst)
            if len(lst) != len(ts):
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {lname} has {len(lst)} tensors, the weights have {len(ts)}")
            checked[lname] = [self._f32(who, f"{lname}[{name}]", t, p.shape) for name, t, p in zip(self.NEUMF_TENSORS, lst, ts)]
        if (not isinstance(triples, torch.Tensor) or triples.dtype != torch.int32 or triples.device != self.device or not triples.is_contiguous()
                or triples.dim() != 2 or triples.shape[1] != 3):
            raise SdrmError(f"{who}: triples must be a contiguous int32 tensor [n, 3] on the engine's device")
        n, batch, step0 = int(triples.shape[0]), int(batch), int(step0)
        if n < 1 or n > 2 ** 31 - 1 or batch < 1 or batch > self.NEUMF_TRAIN_MAX_BATCH:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n = {n} outside 1 .. 2^31 - 1 or batch = {batch} outside 1 .. {self.NEUMF_TRAIN_MAX_BATCH}")
        if step0 < 0 or not (0.0 <= float(p_drop) < 1.0):
            raise SdrmError(f"{who}: SDRM_ERR_ARG: step0 = {step0} < 0 or p_drop = {p_drop} outside [0, 1)")
        mode = 1
        if keep is not None:
            if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.uint8 or keep.device != self.device or not keep.is_contiguous()
                    or tuple(keep.shape) != (n, 14 * F)):
                raise SdrmError(f"{who}: keep must be a contiguous uint8 tensor [{n}, {14 * F}] on the engine's device")
            mode = 0
        rec = _lib.NeumfTrain()
        for i in range(len(ts)):
            rec.p[i], rec.m[i], rec.v[i] = ts[i].data_ptr(), checked["exp_avg"][i].data_ptr(), checked["exp_avg_sq"][i].data_ptr()
        rec.n_users, rec.n_items, rec.factor = n_users, n_items, F
        gptr = None
        if grads is not None:
            gptr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in checked["grads"]])
        losses = torch.empty(-(-n // batch), dtype=torch.float64, device=self.device)
        self._check(self.lib.sdrm_neumf_train_steps(self._h, C.byref(rec), _ptr(triples), n, batch, step0, float(lr), float(betas[0]), float(betas[1]),
                                                    float(eps), float(p_drop), mode, _ptr(keep), int(seed) & (2 ** 64 - 1), int(call_id) & 0xFFFFFFFF,
                                                    _ptr(losses), gptr, _stream()), "sdrm_neumf_train_steps")
        if check:
            self.feed_status()
        return losses

    # ------------------------------------------------------------------ NeuMF evaluator's epoch draw (csrc/neumf_draw.h)
    def neumf_epoch_draw(self, triples, n_hold=None, seed=0, epoch=0, n_users=None, out=None):
        """neural_cf_benchmark_pt.py:180-184 on the device (sdrm_neumf_epoch_draw): an epoch's 80/20 split of `triples` (int32 device
        tensor [n, 3]: user, item, label; left as it is), the label-0 rows of the 80 % drawn again with replacement, one per label-1 row,
        and the shuffle of both - a function of (seed, epoch) and the triples alone, defined in include/sdrm_hip.h and restated in
        tests/neumf_draw_ref.py; never numpy's or torch's generator.  `n_hold`: rows of the hold-out part, default ceil(0.2 n).
        Returns (hold, part, counts, present): hold int32 [n_hold, 3]; part the view [:m] of an int32 [2 (n - n_hold), 3] buffer, what
        `neumf_train_steps` takes; counts the Python tuple (n_pos, n_neg, m); present a uint8 device tensor [n_users], 1 for every user id
        of hold inside [0, n_users) (an id outside raises the feed status word's row bit: ask `feed_status`), or None without `n_users`.
        `out`: (hold buffer [n_hold, 3], part buffer [>= 2 (n - n_hold), 3]) to fill, so that a driver reuses both across epochs; rows of
        the part buffer behind m keep what they held.  The call is DEVICE-SYNCHRONOUS and takes no stream: it waits for every stream before it starts and for its own work
        before it returns, so it cannot run under graph capture."""
        who = "neumf_epoch_draw"
        if (not isinstance(triples, torch.Tensor) or triples.dtype != torch.int32 or triples.device != self.device or not triples.is_contiguous()
                or triples.dim() != 2 or triples.shape[1] != 3):
            raise SdrmError(f"{who}: triples must be a contiguous int32 tensor [n, 3] on the engine's device")
        n = int(triples.shape[0])
        n_hold = int(math.ceil(0.2 * n)) if n_hold is None else int(n_hold)
        if n < 2 or n > 2 ** 30 or n_hold < 1 or n_hold >= n:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n = {n} outside 2 .. 2^30 or n_hold = {n_hold} outside 1 .. n - 1")
        if n_users is not None and int(n_users) < 1:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_users = {n_users} < 1")
        cap = 2 * (n - n_hold)
        if out is None:
            out = (torch.empty(n_hold, 3, dtype=torch.int32, device=self.device), torch.empty(cap, 3, dtype=torch.int32, device=self.device))
        hold, buf = out
        for name, t, rows in (("out[0]", hold, n_hold), ("out[1]", buf, cap)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous()
                    or t.dim() != 2 or t.shape[1] != 3 or (t.shape[0] != rows if name == "out[0]" else t.shape[0] < rows)):
                raise SdrmError(f"{who}: {name} must be a contiguous int32 tensor [{'' if name == 'out[0]' else '>= '}{rows}, 3] on the engine's device")
        present = None if n_users is None else torch.empty(int(n_users), dtype=torch.uint8, device=self.device)
        counts = (C.c_int64 * 3)()
        self._check(self.lib.sdrm_neumf_epoch_draw(self._h, _ptr(triples), n, n_hold, int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF, _ptr(hold),
                                                   _ptr(buf), int(buf.shape[0]), _ptr(present), 0 if n_users is None else int(n_users), counts),
                    "sdrm_neumf_epoch_draw")
        n_pos, n_neg, m = (int(c) for c in counts)
        return hold, buf[:m], (n_pos, n_neg, m), present

    # ------------------------------------------------------------------ NeuMF evaluator's triples from CSR parts (csrc/neumf_triples.h)
    NEUMF_TRIPLES_MAX = 2 ** 30   # rows of the triple buffer: neumf_epoch_draw's bound on n

    def neumf_triples(self, parts, n_items, out=None, present=True, check=True):
        """main.py:218-283's frames and `concat` on the device (sdrm_neumf_triples): the (user, item, label) triples of up to 8 device CSR
        parts, in the order include/sdrm_hip.h defines - parts as given, rows ascending, entries in their stored order, dense.  `parts`: a
        list of (device CSR tuple as `equal_sparsity_csr` / `csr_to_device` / `holdout_split` return, user0, label): row r of the part is
        user user0 + r, label is 0 or 1; only the pattern is read, values are ignored.  `n_items`: the width every part is held to.
        Returns (triples, counts, item_present): triples the int32 view [m, 3] of `out` or of a fresh buffer with the summed capacities
        as rows - what `neumf_epoch_draw` takes; counts the Python tuple (m, label-1 triples, max user + 1, max item + 1), the ONE
        readback, 32 bytes, which also sizes the view; item_present a uint8 device tensor [n_items], 1 for every item that occurs (None
        with `present=False`).  `out`: a contiguous int32 device tensor [>= summed capacities, 3] to fill; rows behind m keep what they
        held.  A row with a bad indptr pair or a column outside [0, n_items) is EMPTY in the output and raises the feed status word
        (`check` as in `csr_rows_to_dense`)."""
        who = "neumf_triples"
        parts = list(parts)
        if not 1 <= len(parts) <= self.CSR_STACK_MAX:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {len(parts)} parts, outside 1 .. {self.CSR_STACK_MAX}")
        n_items = int(n_items)
        arrays = []
        for i, p in enumerate(parts):
            if not isinstance(p, (tuple, list)) or len(p) != 3:
                raise SdrmError(f"{who}: part {i} must be (device CSR tuple, user0, label)")
            indptr, indices, _, n_rows, n_cols, cap = self._csr_arrays(who, f"part {i}", p[0])
            user0, label = int(p[1]), int(p[2])
            if n_cols > n_items:
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: part {i} has {n_cols} columns, n_items is {n_items}")
            if label not in (0, 1) or user0 < 0 or user0 + n_rows > 2 ** 31 - 1:
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: part {i}: label {label} outside {{0, 1}}, or users {user0} .. {user0 + n_rows - 1} outside int32")
            arrays.append((indptr, indices, n_rows, cap, user0, label))
        rows, capacity = sum(a[2] for a in arrays), sum(a[3] for a in arrays)
        if not (1 <= rows <= 2 ** 22 and 1 <= n_items <= 2 ** 22) or capacity > self.NEUMF_TRIPLES_MAX:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {rows} rows or {n_items} items outside 1 .. 2^22, or {capacity} entries above 2^30")
        if out is None:
            out = torch.empty(max(capacity, 1), 3, dtype=torch.int32, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != self.device or not out.is_contiguous() or out.dim() != 2
                or out.shape[1] != 3 or not max(capacity, 1) <= out.shape[0] <= self.NEUMF_TRIPLES_MAX):
            raise SdrmError(f"{who}: out must be a contiguous int32 tensor [{max(capacity, 1)} .. 2^30, 3] on the engine's device")
        item_present = torch.empty(n_items, dtype=torch.uint8, device=self.device) if present else None
        counts_dev = torch.empty(4, dtype=torch.int64, device=self.device)
        desc = (_lib.TriplePart * len(arrays))()
        for d, (ip, ix, n_rows, cap, user0, label) in zip(desc, arrays):
            d.indptr, d.indices = ip.data_ptr(), ix.data_ptr() if cap else None   # (an empty tensor has no address; the ABI takes null with capacity 0)
            d.n_rows, d.capacity, d.user0, d.label = n_rows, cap, user0, label
        self._check(self.lib.sdrm_neumf_triples(self._h, desc, len(arrays), n_items, _ptr(out), int(out.shape[0]), _ptr(item_present), _ptr(counts_dev),
                                                _stream()), "sdrm_neumf_triples")
        self._feed_keep = arrays
        counts = tuple(int(c) for c in counts_dev.cpu().tolist())
        if check:
            self.feed_status()
        return out[:counts[0]], counts, item_present

    # ------------------------------------------------------------------ NeuMF evaluator's ranking problem on the device (csrc/neumf_rank.h)
    def neumf_rank_problem(self, parts, n_items, item_present, heldout, n_rows, check=True):
        """neural_cf_benchmark_pt.py:294-326's ranking problem on the device (sdrm_neumf_rank_problem; include/sdrm_hip.h defines it,
        tests/neumf_rank_ref.py restates it): what `neumf.RankingProblem.from_parts` builds on the host, with the rows of both matrices
        dense by user id.  `parts`, `n_items`: as `neumf_triples` takes them; `item_present`: the uint8 device tensor [n_items] that call
        returned; `heldout`: int32 device tensor [n, 3] of (user, item, label) triples, n may be 0; `n_rows`: the number of user ids.
        Returns a `NeumfRankProblem`; its counts are the call's ONE readback, 32 bytes, which also sizes the views.  A part row that
        fails `neumf_triples`' checks contributes nothing, a held-out triple with a user outside [0, n_rows) or an item outside
        [0, n_items) is dropped, and either raises the feed status word (`check` as in `csr_rows_to_dense`)."""
        who = "neumf_rank_problem"
        parts = list(parts)
        if not 1 <= len(parts) <= self.CSR_STACK_MAX:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {len(parts)} parts, outside 1 .. {self.CSR_STACK_MAX}")
        n_items, n_rows = int(n_items), int(n_rows)
        arrays = []
        for i, p in enumerate(parts):
            if not isinstance(p, (tuple, list)) or len(p) != 3:
                raise SdrmError(f"{who}: part {i} must be (device CSR tuple, user0, label)")
            indptr, indices, _, rows_p, n_cols, cap = self._csr_arrays(who, f"part {i}", p[0])
            user0, label = int(p[1]), int(p[2])
            if n_cols > n_items:
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: part {i} has {n_cols} columns, n_items is {n_items}")
            if label not in (0, 1) or user0 < 0 or user0 + rows_p > 2 ** 31 - 1:
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: part {i}: label {label} outside {{0, 1}}, or users {user0} .. {user0 + rows_p - 1} outside int32")
            arrays.append((indptr, indices, rows_p, cap, user0, label))
        rows, capacity = sum(a[2] for a in arrays), sum(a[3] for a in arrays)
        if (not (1 <= rows <= 2 ** 22 and 1 <= n_items <= 2 ** 22 and 1 <= n_rows <= 2 ** 22) or capacity > self.NEUMF_TRIPLES_MAX
                or n_rows * -(-n_items // 64) * 8 > 2 ** 31):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {rows} part rows, {n_items} items or {n_rows} users outside 1 .. 2^22, {capacity} entries above "
                            f"2^30, or a bit table above 2^31 bytes")
        if (not isinstance(item_present, torch.Tensor) or item_present.dtype != torch.uint8 or item_present.device != self.device
                or not item_present.is_contiguous() or tuple(item_present.shape) != (n_items,)):
            raise SdrmError(f"{who}: item_present must be a contiguous uint8 tensor [{n_items}] on the engine's device")
        if (not isinstance(heldout, torch.Tensor) or heldout.dtype != torch.int32 or heldout.device != self.device or not heldout.is_contiguous()
                or heldout.dim() != 2 or heldout.shape[1] != 3 or heldout.shape[0] > 2 ** 30):
            raise SdrmError(f"{who}: heldout must be a contiguous int32 tensor [0 .. 2^30, 3] on the engine's device")
        n_held = int(heldout.shape[0])
        cols = torch.empty(n_items, dtype=torch.int32, device=self.device)
        seen_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        seen_idx = torch.empty(max(capacity, 1), dtype=torch.int32, device=self.device)
        rel_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        rel_idx = torch.empty(max(n_held, 1), dtype=torch.int32, device=self.device)
        counts_dev = torch.empty(4, dtype=torch.int64, device=self.device)
        desc = (_lib.TriplePart * len(arrays))()
        for d, (ip, ix, rows_p, cap, user0, label) in zip(desc, arrays):
            d.indptr, d.indices = ip.data_ptr(), ix.data_ptr() if cap else None   # (an empty tensor has no address; the ABI takes null with capacity 0)
            d.n_rows, d.capacity, d.user0, d.label = rows_p, cap, user0, label
        self._check(self.lib.sdrm_neumf_rank_problem(self._h, desc, len(arrays), n_items, _ptr(item_present), _ptr(heldout) if n_held else None, n_held,
                                                     n_rows, _ptr(cols), n_items, _ptr(seen_ptr), _ptr(seen_idx), int(seen_idx.numel()), _ptr(rel_ptr),
                                                     _ptr(rel_idx), int(rel_idx.numel()), _ptr(counts_dev), _stream()), "sdrm_neumf_rank_problem")
        self._feed_keep = (arrays, item_present, heldout)
        counts = tuple(int(c) for c in counts_dev.cpu().tolist())
        if check:
            self.feed_status()
        C_, shape = counts[0], (n_rows, counts[0])
        return NeumfRankProblem(cols[:C_], (seen_ptr, seen_idx[:counts[1]], None, shape), (rel_ptr, rel_idx[:counts[2]], None, shape), counts)

    def neumf_rank_users(self, mask):
        """The ascending int32 user list of a uint8 device mask [n_rows] (sdrm_neumf_rank_users): `np.flatnonzero` of the bytes
        `neumf_epoch_draw` leaves in `present`, on the device.  Returns the view [U]; U is the call's one readback, 8 bytes (it sizes the
        score matrix of the ranking that follows)."""
        who = "neumf_rank_users"
        if (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 1 or mask.device != self.device
                or not mask.is_contiguous()):
            raise SdrmError(f"{who}: mask must be a contiguous 1-D uint8 tensor on the engine's device")
        n_rows = int(mask.numel())
        if not 1 <= n_rows <= 2 ** 22:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {n_rows} users, outside 1 .. 2^22")
        users = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        count_dev = torch.empty(1, dtype=torch.int64, device=self.device)
        self._check(self.lib.sdrm_neumf_rank_users(self._h, _ptr(mask), n_rows, _ptr(users), _ptr(count_dev), _stream()), "sdrm_neumf_rank_users")
        return users[:int(count_dev.cpu().item())]

    def rank_metrics_rows(self, scores, rows, heldout, train=None, ks=(1, 3, 5, 10, 20, 50), full_idcg=False):
        """`rank_metrics` for score rows that are a SELECTION of the rows of two resident matrices (sdrm_rank_metrics_rows): score row q of
        the float32 device matrix [U, I] ranks against CSR row rows[q] (int32 device tensor [U], any order, repeats allowed) of the device
        CSR tuples `heldout` and `train` [n_rows, I] - no gather of either.  Every row id, offset and column is range-checked on the
        device into the feed status word (ask `feed_status()`).  `full_idcg=True`: the NDCG on the NeuMF evaluator's footing, ideal DCG
        of min(I, k) items for every user and 0 without a relevant item - the bits `neumf.rank_all_items` makes on the host.  The discount
        tables come from the per-`ks` cache `rank_metrics` uses.  Returns (recall [nk, U], ndcg [nk, U]) float64 device tensors."""
        who = "rank_metrics_rows"
        if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
            raise SdrmError(f"{who}: scores must be a float32 device matrix [U, I]")
        scores = self._f32(who, "scores", scores, tuple(scores.shape))
        U, I = (int(v) for v in scores.shape)
        if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != self.device or not rows.is_contiguous()
                or rows.numel() != U):
            raise SdrmError(f"{who}: rows must be a contiguous int32 tensor [{U}] on the engine's device")
        if train is not None and not isinstance(train, tuple):
            raise SdrmError(f"{who}: heldout and train are device CSR tuples")
        n_rows = int(heldout[3][0])

        def matrix(name, csr_dev):
            indptr, indices, _, rows_m, width, cap = self._csr_arrays(who, name, csr_dev)
            if width != I or rows_m != n_rows:
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: the {name} matrix is {rows_m} x {width}, the scores have {I} columns and the held-out matrix {n_rows} rows")
            return indptr, indices if cap else indices.new_zeros(1), cap
        hp, hi, hn = matrix("held-out", heldout)
        tp_, ti, tn = matrix("train", train) if train is not None else (None, None, 0)
        ks_h, tp_d, idcg_d = self._rank_tables(ks)
        recall = torch.empty(len(ks_h), U, dtype=torch.float64, device=self.device)
        ndcg = torch.empty(len(ks_h), U, dtype=torch.float64, device=self.device)
        if U == 0:
            return recall, ndcg
        self._check(self.lib.sdrm_rank_metrics_rows(self._h, _ptr(scores), U, I, _ptr(rows), n_rows, _ptr(hp), _ptr(hi), hn, _ptr(tp_), _ptr(ti), tn,
                                                    ks_h.ctypes.data_as(C.c_void_p), len(ks_h), _ptr(tp_d), _ptr(idcg_d), _ptr(recall), _ptr(ndcg),
                                                    int(bool(full_idcg)), _stream()), "sdrm_rank_metrics_rows")
        self._keepalive = (scores, rows, hp, hi, tp_, ti)
        return recall, ndcg

    # ------------------------------------------------------------------ MLP evaluator's train steps (csrc/mlp_train.h)
    MLP_TENSORS = ("mf_embedding_user", "layer1/kernel", "layer1/bias", "layer2/kernel", "layer2/bias", "layer3/kernel", "layer3/bias",
                   "prediction/kernel", "prediction/bias")
    MLP_WIDTHS = (512, 256, 256)
    MLP_FACTORS = 8
    MLP_MAX_BATCH = 16
    MLP_MAX_ITEMS = 36864

    @classmethod
    def mlp_shapes(cls, n_users, n_items):
        """The nine shapes of the MLP evaluator's tensors in Keras's `get_weights()` order (`MLP_TENSORS`), kernels [in, out]."""
        h1, h2, h3 = cls.MLP_WIDTHS
        return ((n_users, cls.MLP_FACTORS), (cls.MLP_FACTORS * n_items, h1), (h1,), (h1, h2), (h2,), (h2, h3), (h3,), (h3, n_items), (n_items,))

    def mlp_train_steps(self, weights, exp_avg, exp_avg_sq, csr_dev, rows, batch=16, step0=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, p_drop=0.5,
                        seed=0, call_id=0, keep=None, grads_out=None, check=True):
        """The batch loop of the MLP evaluator's `model.fit` (mlp_benchmark.py:102-107) on the device (sdrm_mlp_train_steps): ceil(n / batch)
        consecutive train steps over the rows `rows` (int64 device tensor [n]) of the 0 / 1 matrix `csr_dev` (a `csr_to_device` tuple; only
        its pattern is read) in order, the last batch partial - train-mode forward with the three dropouts, binary cross-entropy from the
        logits over all b n_items elements, the gradients of all nine tensors and Keras's Adam (eps beside sqrt(v)), all enqueued by this
        one call with no host synchronisation.  `weights`: the nine live float32 tensors in `MLP_TENSORS` order and `mlp_shapes`' shapes
        (`mlp_eval.MLP.engine_weights()`), UPDATED IN PLACE; `exp_avg`, `exp_avg_sq`: nine tensors of the same shapes, updated in place;
        every one starts on a 16-byte boundary and no two share a byte.  Adam's step count for step t of the call is `step0 + t + 1`.
        Dropout: with `keep` (uint8 device tensor [n, 1024]: 512 + 256 + 256 columns, non-zero = kept) the masks are the caller's; without,
        they are Philox4x32-10's of (seed, call_id, the row's place in `rows`, column).  `grads_out`: nine float32 tensors of the weights'
        shapes that receive the gradients the update used - for a call of ONE step only.  Row ids and column indices are range-checked on
        the device (`check` as in `csr_rows_to_dense`).  Returns the per-step losses, a float64 device tensor [ceil(n / batch)]."""
        who = "mlp_train_steps"
        lists = {"weights": weights, "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
        if grads_out is not None:
            lists["grads_out"] = grads_out
        for lname, lst in lists.items():
            lst = list(lst.values()) if isinstance(lst, dict) else list(lst)
            if len(lst) != len(self.MLP_TENSORS):
                raise SdrmError(f"{who}: SDRM_ERR_SHAPE: {lname} has {len(lst)} tensors; the model has nine ({', '.join(self.MLP_TENSORS)})")
            lists[lname] = lst
        e, w1 = lists["weights"][0], lists["weights"][1]
        if not isinstance(e, torch.Tensor) or e.dim() != 2 or not isinstance(w1, torch.Tensor) or w1.dim() != 2 or w1.shape[0] % self.MLP_FACTORS:
            raise SdrmError(f"{who}: {self.MLP_TENSORS[0]} must be a 2-D tensor [n_users, 8] and {self.MLP_TENSORS[1]} one [8 n_items, 512]")
        n_users, n_items = int(e.shape[0]), int(w1.shape[0]) // self.MLP_FACTORS
        shapes = self.mlp_shapes(n_users, n_items)
        checked = {lname: [self._f32(who, f"{lname}[{name}]", t.detach() if isinstance(t, torch.Tensor) else t, shape)
                           for name, t, shape in zip(self.MLP_TENSORS, lst, shapes)] for lname, lst in lists.items()}
        indptr, indices, _, m_rows, m_cols, _ = self._sparse_dev(who, "csr", csr_dev)
        if m_cols != n_items:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: the matrix has {m_cols} columns, the model {n_items} items")
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.device != self.device or not rows.is_contiguous() or rows.dim() != 1:
            raise SdrmError(f"{who}: rows must be a contiguous 1-D int64 tensor on the engine's device")
        n, batch, step0 = int(rows.numel()), int(batch), int(step0)
        if (not 1 <= n_items <= self.MLP_MAX_ITEMS or n_users < 2 or m_rows < 1 or not 1 <= n <= 2 ** 31 - 1 or not 1 <= batch <= self.MLP_MAX_BATCH
                or step0 < 0 or not (0.0 <= float(p_drop) < 1.0)):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: n_items = {n_items} outside 1 .. {self.MLP_MAX_ITEMS}, n_users = {n_users} < 2, no row, n = {n} "
                            f"outside 1 .. 2^31 - 1, batch = {batch} outside 1 .. {self.MLP_MAX_BATCH}, step0 = {step0} < 0 or p_drop = {p_drop} "
                            f"outside [0, 1)")
        mode = 1
        if keep is not None:
            if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.uint8 or keep.device != self.device or not keep.is_contiguous()
                    or tuple(keep.shape) != (n, sum(self.MLP_WIDTHS))):
                raise SdrmError(f"{who}: keep must be a contiguous uint8 tensor [{n}, {sum(self.MLP_WIDTHS)}] on the engine's device")
            mode = 0
        rec = _lib.MlpTrain()
        for i in range(len(self.MLP_TENSORS)):
            rec.p[i], rec.m[i], rec.v[i] = (checked[k][i].data_ptr() for k in ("weights", "exp_avg", "exp_avg_sq"))
        rec.n_users, rec.n_items = n_users, n_items
        gptr = None
        if grads_out is not None:
            gptr = (C.c_void_p * len(self.MLP_TENSORS))(*[t.data_ptr() for t in checked["grads_out"]])
        losses = torch.empty(-(-n // batch), dtype=torch.float64, device=self.device)
        self._check(self.lib.sdrm_mlp_train_steps(self._h, C.byref(rec), _ptr(indptr), _ptr(indices), m_rows, _ptr(rows), n, batch, step0, float(lr),
                                                  float(betas[0]), float(betas[1]), float(eps), float(p_drop), mode, _ptr(keep),
                                                  int(seed) & (2 ** 64 - 1), int(call_id) & 0xFFFFFFFF, _ptr(losses), gptr, _stream()),
                    "sdrm_mlp_train_steps")
        self._feed_keep = (indptr, indices, rows, keep, checked)
        if check:
            self.feed_status()
        return losses

    # ------------------------------------------------------------------ MLP evaluator's eval-mode forward (csrc/mlp_eval.h)
    MLP_EVAL_MAX_BATCH = 4096

    def mlp_eval(self, weights, csr_dev, rows=None, row0=0, n=None, batch=1024, logits=False, out=None, sse=False, check=True):
        """`model.predict` (mlp_benchmark.py:114) and the numerator of the validation `RootMeanSquaredError` (:92, :109) on the device
        (sdrm_mlp_eval): the model's inference-mode forward for the rows `rows` (int64, any order, repeats allowed) or row0 .. row0 + n - 1
        (default: up to the last row) of the 0 / 1 matrix `csr_dev` (a `csr_to_device` tuple; only its pattern is read), in batches of
        `batch` rows inside the one call, with no dense input and ONE pass over W1.  `weights`: the nine live float32 tensors as
        `mlp_train_steps` takes them, read in place.  `out`: None - a new float32 [n, n_items] -, a tensor of that shape to fill, or False:
        no output of that size exists anywhere.  It receives sigmoid(y), or the logits y with `logits=True`.  `sse=True`: also a float64
        device tensor of ONE element, the sum over all n x n_items elements of (sigmoid(y) - x)^2, whatever `logits` says.  Returns `out`,
        `(out, sse_tensor)`, or `sse_tensor` alone when `out is False`.  Nothing is read back; row ids, indptr pairs and column indices
        are range-checked on the device (a bad row is zero in `out` and absent from the sum; `check` as in `csr_rows_to_dense`)."""
        who = "mlp_eval"
        lst = list(weights.values()) if isinstance(weights, dict) else list(weights)
        if len(lst) != len(self.MLP_TENSORS):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: weights has {len(lst)} tensors; the model has nine ({', '.join(self.MLP_TENSORS)})")
        e, w1 = lst[0], lst[1]
        if not isinstance(e, torch.Tensor) or e.dim() != 2 or not isinstance(w1, torch.Tensor) or w1.dim() != 2 or w1.shape[0] % self.MLP_FACTORS:
            raise SdrmError(f"{who}: {self.MLP_TENSORS[0]} must be a 2-D tensor [n_users, 8] and {self.MLP_TENSORS[1]} one [8 n_items, 512]")
        n_users, n_items = int(e.shape[0]), int(w1.shape[0]) // self.MLP_FACTORS
        checked = [self._f32(who, f"weights[{name}]", t.detach() if isinstance(t, torch.Tensor) else t, shape)
                   for name, t, shape in zip(self.MLP_TENSORS, lst, self.mlp_shapes(n_users, n_items))]
        indptr, indices, _, m_rows, m_cols, nnz = self._sparse_dev(who, "csr", csr_dev)
        if m_cols != n_items:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: the matrix has {m_cols} columns, the model {n_items} items")
        if rows is not None:
            if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.device != self.device or not rows.is_contiguous() or rows.dim() != 1:
                raise SdrmError(f"{who}: rows must be a contiguous 1-D int64 tensor on the engine's device")
            n = int(rows.numel())
        elif n is None:
            n = m_rows - int(row0)
        n, row0, batch = int(n), int(row0), int(batch)
        if out is False and not sse:
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: out=False without sse=True asks for nothing")
        rc = self.lib.sdrm_debug_mlp_eval_args(n_users, n_items, nnz, m_rows, int(rows is not None), row0, n, batch, int(out is not False), int(bool(sse)),
                                               None, 0)
        if rc:
            raise SdrmError(f"{who}: {_lib.STATUS.get(rc, rc)}: n_items = {n_items} outside 1 .. {self.MLP_MAX_ITEMS}, n_users = {n_users} < 2, batch = "
                            f"{batch} outside 1 .. {self.MLP_EVAL_MAX_BATCH}, n = {n} < 1, rows {row0} .. {row0 + n - 1} outside the matrix's {m_rows}, or "
                            f"n x n_items at or above 2^40")
        if out is None:
            out = torch.empty(n, n_items, dtype=torch.float32, device=self.device)
        elif out is not False:
            out = self._f32(who, "out", out, (n, n_items))
        sse_t = torch.empty(1, dtype=torch.float64, device=self.device) if sse else None
        rec = _lib.MlpEvalW()
        for i, t in enumerate(checked):
            rec.p[i] = t.data_ptr()
        rec.n_users, rec.n_items = n_users, n_items
        self._check(self.lib.sdrm_mlp_eval(self._h, C.byref(rec), _ptr(indptr), _ptr(indices), nnz, m_rows, _ptr(rows), row0, n, batch, int(bool(logits)),
                                           _ptr(out) if out is not False else None, _ptr(sse_t), _stream()), "sdrm_mlp_eval")
        self._feed_keep = (indptr, indices, rows, checked)
        if check:
            self.feed_status()
        if out is False:
            return sse_t
        return (out, sse_t) if sse else out

    # ------------------------------------------------------------------ evaluation half of the VAE pre-stage (csrc/eval_half.h)
    def vae_eval_holdout(self, w1, b1, w2, b2, w3, b3, w4, b4, train_csr_dev, held_csr_dev, k, metric, batch=500, out=None, logits=None,
                         check=False):
        """train_SDRM.py:160-177 in eval mode for every user of a hold-out split, in one engine call (sdrm_vae_eval_holdout): the VAE's
        forward - normalise, encoder (mu rows only; no KL, no draw), decoder - straight from the rows of `train_csr_dev`, and `metric`
        ("recall" / 0 or "ndcg" / 1) at cut-off `k` of its scores against `held_csr_dev` with the train items at -inf, as `rank_metrics`
        defines it.  The eight tensors are the live `nn.Linear` weights and biases (encoder[0], encoder[2], decoder[0], decoder[2]),
        float32 and contiguous on the engine's device; the two CSRs are `(indptr, indices, None, shape)` tuples as `holdout_split`
        returns them.  The weights are staged once, the call loops over batches of `batch` users itself, and no dense input batch exists.
        Returns the float64 device tensor [n_rows] of per-user scores (`out`, when given) - nan for a user with nothing held out.
        `logits`: a float32 device tensor [n_rows, n_items] that receives the scores of every item; without it nothing of that size is
        allocated.  Nothing is read back; `check=True` asks `feed_status()` at once."""
        who = "vae_eval_holdout"
        if isinstance(metric, str) and metric in ("recall", "Recall"):
            metric = 0
        elif isinstance(metric, str) and metric in ("ndcg", "NDCG"):
            metric = 1
        elif isinstance(metric, (bool, str)) or not isinstance(metric, (int, np.integer)) or int(metric) not in (0, 1):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: metric = {metric!r} is none of \"recall\" / 0 and \"ndcg\" / 1")
        tr_ptr, tr_idx, _, (n_rows, n_items) = train_csr_dev
        he_ptr, he_idx, _, he_shape = held_csr_dev
        n_rows, n_items = int(n_rows), int(n_items)
        if (int(he_shape[0]), int(he_shape[1])) != (n_rows, n_items):
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: the held part is {tuple(he_shape)}, the train part {(n_rows, n_items)}")
        if not isinstance(w1, torch.Tensor) or w1.dim() != 2 or not isinstance(w3, torch.Tensor) or w3.dim() != 2:
            raise SdrmError(f"{who}: w1 must be a 2-D tensor [hidden, n_items] and w3 one [hidden, latent]")
        hidden, latent = int(w3.shape[0]), int(w3.shape[1])
        w1 = self._f32(who, "w1", w1.detach(), (hidden, n_items))
        b1 = self._f32(who, "b1", b1.detach(), (hidden,))
        w2 = self._f32(who, "w2", w2.detach(), (2 * latent, hidden))
        b2 = self._f32(who, "b2", b2.detach(), (2 * latent,))
        w3 = self._f32(who, "w3", w3.detach(), (hidden, latent))
        b3 = self._f32(who, "b3", b3.detach(), (hidden,))
        w4 = self._f32(who, "w4", w4.detach(), (n_items, hidden))
        b4 = self._f32(who, "b4", b4.detach(), (n_items,))
        tr_ptr = self._index(who, "train indptr", tr_ptr, torch.int64, n_rows + 1)
        he_ptr = self._index(who, "held indptr", he_ptr, torch.int64, n_rows + 1)
        nnz = []
        idx = []
        for name, t in (("train", tr_idx), ("held", he_idx)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
                raise SdrmError(f"{who}: {name} indices must be a contiguous int32 tensor on the engine's device")
            nnz.append(int(t.numel()))
            idx.append(t.new_zeros(1) if t.numel() == 0 else t)   # torch gives an empty tensor no address, and the C ABI takes no null array
        if out is None:
            out = torch.empty(n_rows, dtype=torch.float64, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous() \
                or tuple(out.shape) != (n_rows,):
            raise SdrmError(f"{who}: out must be a contiguous float64 tensor [{n_rows}] on the engine's device")
        if logits is not None:
            logits = self._f32(who, "logits", logits, (n_rows, n_items))
        if not 1 <= int(k) <= min(128, n_items):   # (the tables below are made for k: the C call's own refusal would come too late)
            raise SdrmError(f"{who}: SDRM_ERR_SHAPE: k = {k} outside 1 .. min(128, n_items)")
        _, tp_d, idcg_d = self._rank_tables((int(k),))
        enc = _lib.VaeEncoder(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), n_items, hidden, latent)
        dec = _lib.VaeDecoder(w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(), latent, hidden, n_items)
        self._check(self.lib.sdrm_vae_eval_holdout(self._h, C.byref(enc), C.byref(dec), _ptr(tr_ptr), _ptr(idx[0]), nnz[0], _ptr(he_ptr),
                                                   _ptr(idx[1]), nnz[1], n_rows, int(batch), int(k), _ptr(tp_d), _ptr(idcg_d), int(metric),
                                                   _ptr(out), _ptr(logits), _stream()), "sdrm_vae_eval_holdout")
        self._keepalive = (w1, b1, w2, b2, w3, b3, w4, b4, idx)
        if check:
            self.feed_status()
        return out

    def perturb_input(self, x, t, noise):
        x, t, noise = self._dev(x, torch.float32), self._dev(t, torch.int64), self._dev(noise, torch.float32)
        out = torch.empty_like(x)
        self._check(self.lib.sdrm_perturb_input(self._h, _ptr(x), _ptr(t), _ptr(noise), x.shape[0], _ptr(out), _stream()),
                    "sdrm_perturb_input")
        return out


_UTILITY = {}


def utility_engine(device=None) -> Engine:
    """A small cached engine for the handle-independent device ops (equal_sparsity, rank_metrics, csr_rows_to_dense):
    the C ABI hangs error strings and the select workspace on a handle, nothing of the eps-net is used."""
    idx = torch.cuda.current_device() if device is None else (torch.device(device).index or 0)
    eng = _UTILITY.get(idx)
    if eng is None or not eng._h:
        eng = _UTILITY[idx] = Engine(8, 8, 4, 0, 16, device=idx)
    return eng
