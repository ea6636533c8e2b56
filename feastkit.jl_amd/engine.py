"""HipEngine: the device side of the ``:hip`` backend -- a thin object over the C ABI
(include/feasthip.h).  PyTorch is used only as plumbing: device allocations, the current
HIP stream and ``torch.distributed`` (RCCL) for the per-loop all-reduce of Q_proj.

Block vectors live on the device as COLUMN-MAJOR N x m complex128, i.e. a contiguous
torch tensor of shape (m, N) -- the layout of the reference's Julia ``Matrix{ComplexF64}``.

There is no CPU fallback: constructing a HipEngine without libfeasthip.so or without a
visible MI355X raises ``FeastHipUnavailable``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FeastHipStats, FeastHipUnavailable
from .types import FeastHipError

SOLVER_LU, SOLVER_BICGSTAB, SOLVER_GMRES, SOLVER_COCG, SOLVER_BANDED, SOLVER_SHIFTED_COCG, SOLVER_BLOCK_COCG = 0, 1, 2, 3, 4, 5, 6
_SOLVER_CODES = {"direct": SOLVER_LU, "lu": SOLVER_LU, "bicgstab": SOLVER_BICGSTAB,
                 "iterative": SOLVER_BICGSTAB, "gmres": SOLVER_GMRES, "cocg": SOLVER_COCG,
                 "banded": SOLVER_BANDED, "shifted_cocg": SOLVER_SHIFTED_COCG, "block_cocg": SOLVER_BLOCK_COCG}
MAX_BLOCK = 64   # FH_MAX_LD: widest panel the kernels take in one call


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class HipEngine:
    def __init__(self, device_index: int = 0):
        import torch
        self.torch = torch
        self.lib = _lib.load_library()
        if not torch.cuda.is_available():
            raise FeastHipUnavailable("no HIP device visible (torch.cuda.is_available() is False); "
                                      "feastkit.jl_amd has no CPU fallback")
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        rc = self.lib.feasthip_create(C.byref(h), device_index)
        if rc != 0 or not h:
            raise FeastHipUnavailable(f"feasthip_create(device={device_index}) failed with code {rc}")
        self.h = h
        self._stream_handle = torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.lib.feasthip_set_stream(self.h, C.c_void_p(self._stream_handle)))
        self.N = 0
        self.b_identity = True
        self.last_stats = {}
        self.comm_size, self.comm_rank = 1, 0

    # -- lifecycle ----------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.feasthip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, ok=(0,)):
        op = getattr(self, "_op", None)
        cause = None
        if op is not None:                           # what the operator callback caught during this call, if anything
            cause, op["error"] = op["error"], None
        if rc not in ok:
            msg = self.lib.feasthip_last_error(self.h)
            err = FeastHipError(rc, msg.decode() if msg else "")
            if cause is not None:
                raise err from cause
            raise err
        return rc

    # -- communicator (the collective lives in the C ABI; the host only ships the unique id) -----
    def comm_unique_id(self):
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        self._chk(self.lib.feasthip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks, rank, uid, transport="auto"):
        """Attach rank ``rank`` of ``nranks`` to this handle (collective).  transport: "rccl" (one rank per
        GPU, RCCL over xGMI), "shm" (ranks sharing one device: test rigs), "auto"."""
        code = {"auto": 0, "rccl": 1, "shm": 2}[transport]
        self._chk(self.lib.feasthip_comm_init_rank(self.h, int(nranks), int(rank), bytes(uid), code))
        self.comm_size, self.comm_rank = int(nranks), int(rank)

    def comm_init_from_group(self, group=None, transport="auto"):
        """Convenience for hosts that already run a ``torch.distributed`` group (any backend; it is used as the
        CONTROL plane only): rank 0's unique id is broadcast through it, and ranks that share a HIP device are
        detected so that "auto" picks the shared-device transport for them.  The data plane -- the per-loop sum of
        Q_proj -- is the library's own RCCL all-reduce."""
        import socket
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        if world == 1:
            return
        box = [self.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        props = self.torch.cuda.get_device_properties(self.device)
        ident = (socket.gethostname(), str(getattr(props, "uuid", "")), int(getattr(props, "pci_domain_id", 0)),
                 int(getattr(props, "pci_bus_id", self.device.index)), int(getattr(props, "pci_device_id", 0)))
        idents = [None] * world
        dist.all_gather_object(idents, ident, group=group)
        if transport == "auto":
            transport = "shm" if len(set(idents)) < world else "rccl"
        self.comm_init(world, rank, box[0], transport)

    def comm_transport(self):
        """0 none, 1 RCCL, 2 shared-device (shm)."""
        n, r, t = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.feasthip_comm_info(self.h, C.byref(n), C.byref(r), C.byref(t)))
        return int(t.value)

    def comm_destroy(self):
        self._chk(self.lib.feasthip_comm_destroy(self.h))
        self.comm_size, self.comm_rank = 1, 0

    def set_column_block(self, first=0, count=-1):
        """Columns [first, first+count) of the following contour_apply calls are swept by this rank (count < 0:
        all); the rest arrives through the all-reduce."""
        self._chk(self.lib.feasthip_set_column_block(self.h, int(first), int(count)))

    def allreduce_sum_(self, t):
        """In-place sum over the communicator of a contiguous float64/complex128 device tensor (library RCCL)."""
        if self.comm_size == 1:
            return t
        assert t.is_contiguous() and t.device == self.device
        n = t.numel() * (2 if t.is_complex() else 1)
        self._sync_stream()
        self._chk(self.lib.feasthip_allreduce_sum_dev(self.h, C.c_void_p(t.data_ptr()), n))
        return t

    def barrier(self):
        one = self.torch.ones(1, dtype=self.torch.float64, device=self.device)
        self.allreduce_sum_(one)

    def max_over_ranks(self, value):
        """max of a host scalar over the ranks (sum of a one-hot vector through the library's all-reduce)."""
        if self.comm_size == 1:
            return float(value)
        v = self.torch.zeros(self.comm_size, dtype=self.torch.float64, device=self.device)
        v[self.comm_rank] = float(value)
        return float(self.allreduce_sum_(v).max().item())

    # -- problem ------------------------------------------------------------------
    @staticmethod
    def _fingerprint(M):
        """Content fingerprint of a matrix argument: shape, dtypes and a 128-bit hash over the BYTES of indptr, indices and
        data (position dependent: a permutation of the values on the same pattern, A vs A^T of a structurally symmetric
        matrix, two swapped entries all change it).  A repeated feast() call with the same matrices must not pay the
        ingest (union pattern, chunked rows, upload) again; xxh3 takes 0.2 ms on cfg 3's 341 500 nonzeros."""
        import scipy.sparse as sp
        if M is None:
            return None
        if sp.issparse(M):
            M = M if sp.isspmatrix_csr(M) else None
            if M is None:
                return False                                     # other formats: converted anyway, do not cache
            try:
                import xxhash
                h = xxhash.xxh3_128()
            except ImportError:                                  # pragma: no cover - xxhash ships with the image
                import hashlib
                h = hashlib.blake2b(digest_size=16)
            for a in (M.indptr, M.indices, M.data):
                h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
            return ("csr", M.shape, M.nnz, str(M.data.dtype), str(M.indices.dtype), str(M.indptr.dtype), h.hexdigest())
        return False                                             # dense input: the upload IS the cost, no fingerprint pass

    def set_problem(self, A, B=None):
        import scipy.sparse as sp
        self._op = None                                  # (a set_operator problem ends here)
        if sp.issparse(A):
            fp = (self._fingerprint(A), self._fingerprint(B))
            if fp[0] and fp[1] is not False and fp == getattr(self, "_problem_fp", None) and self.N == A.shape[0]:
                return                                           # the same matrices are resident already
            self._set_csr(A, B)
            self._problem_fp = fp if (fp[0] and fp[1] is not False) else None
        else:
            self._problem_fp = None
            self._set_dense(np.asarray(A), None if B is None else np.asarray(B))

    def _set_dense(self, A, B):
        N = A.shape[0]
        if A.ndim != 2 or A.shape[1] != N:
            raise ValueError("Matrix A must be square")
        if B is not None and B.shape != (N, N):
            raise ValueError("Matrix B must match size of A")
        cplx = np.iscomplexobj(A) or (B is not None and np.iscomplexobj(B))
        dt = np.complex128 if cplx else np.float64
        Af = np.asfortranarray(A, dtype=dt)
        Bf = None if B is None else np.asfortranarray(B, dtype=dt)
        self._chk(self.lib.feasthip_set_dense(self.h, N, int(cplx), _np_ptr(Af), N, _np_ptr(Bf), N))
        self.N, self.b_identity = N, B is None

    def _set_csr(self, A, B):
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        N = A.shape[0]
        if A.shape[1] != N:
            raise ValueError("Matrix A must be square")
        cplx = np.iscomplexobj(A.data) or (B is not None and np.iscomplexobj(sp.csr_matrix(B).data))
        dt = np.complex128 if cplx else np.float64
        pa, ia, va = A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data, dtype=dt)
        if B is not None:
            B = sp.csr_matrix(B)
            if B.shape != A.shape:
                raise ValueError("Matrix B must match size of A")
            pb, ib, vb = B.indptr.astype(np.int64), B.indices.astype(np.int64), np.ascontiguousarray(B.data, dtype=dt)
            nb = len(vb)
        else:
            pb = ib = vb = None
            nb = 0
        self._chk(self.lib.feasthip_set_csr(self.h, N, int(cplx), 0, 0, len(va), _np_ptr(pa), _np_ptr(ia), _np_ptr(va),
                                            nb, _np_ptr(pb), _np_ptr(ib), _np_ptr(vb)))
        self.N, self.b_identity = N, B is None

    def set_operator(self, N, A_mul, B_mul=None, *, real=True, symmetric=False, batched=False):
        """Matrix-free problem (feasthip_set_operator): the engine holds no matrix and calls ``A_mul(Y, X)`` / ``B_mul(Y, X)``
        (``B_mul=None``: B = I) wherever it needs a product; each writes its product into ``Y``, like the reference's
        ``A_mul!(y, x)``.  X and Y are torch views of the library's own panels (no copy), on this engine's device:

        real=True     float64 tensors of shape (N, 2 ld): the real view of the N x ld complex panel (re, im interleaved per
                      column), so a real linear operator is applied once to the real and the imaginary columns alike;
        real=False    complex128 tensors of shape (N, ld);
        batched=True  one call with a leading node dimension, (nodes, N, ...); otherwise one call per node.

        ld is 16, 32 or 64; the columns beyond the block width are padding, which a linear operator may multiply along.
        ``symmetric``: A = A^T and B = B^T (what solver "cocg" needs).  The functions run under the library's stream
        (``torch.cuda.stream(ExternalStream(...))``): torch work they queue is ordered with the library's kernels, and they
        must not synchronise on other streams' results.  A function may return a non-zero int to report failure; an
        exception is caught, the call that needed the product raises FeastHipError and chains it.  Only Krylov solvers
        apply (set_solver "bicgstab" | "cocg" | "gmres"); ``operator_stats()`` counts the calls."""
        N = int(N)
        if N < 1:
            raise ValueError("set_operator: N must be at least 1")
        if not callable(A_mul) or (B_mul is not None and not callable(B_mul)):
            raise ValueError("set_operator: A_mul and B_mul must be callable (B_mul=None: B = I)")

        def count(st, which):
            st["A_calls" if which == 0 else "B_calls"] += 1

        cb, state = self._operator_thunk(N, (A_mul, B_mul), real, batched, {"A_calls": 0, "B_calls": 0}, count)
        flags = (_lib.OP_B_IDENTITY if B_mul is None else 0) | (0 if real else _lib.OP_COMPLEX) | (_lib.OP_SYMMETRIC if symmetric else 0)
        self._sync_stream()
        self._chk(self.lib.feasthip_set_operator(self.h, N, cb, None, flags))
        self._op_thunk = cb                        # the ctypes thunk lives until the next operator replaces it
        self._op = state
        self.N, self.b_identity = N, B_mul is None
        self._problem_fp = None

    def _operator_thunk(self, N, muls, real, batched, counters, count):
        """The ctypes callback of set_operator / set_term_operator and its state: ``muls[which](Y, X)`` on torch views of the
        library's panels under the library's stream; ``count(state, which)`` books the call in ``counters``."""
        import time
        torch = self.torch
        state = {"error": None, "callback_seconds": 0.0, "views": {}, **counters}
        dtype_str, width = ("<f8", 2) if real else ("<c16", 1)

        class _Panel:       # a device pointer as the CUDA array interface: torch.as_tensor wraps it without a copy
            def __init__(self, ptr, nodes, ld, stride):
                self.__cuda_array_interface__ = {"shape": (nodes, N, ld * width), "typestr": dtype_str, "data": (ptr, False),
                                                 "version": 2, "strides": (stride * 16, ld * 16, 16 // width)}

        def view(ptr, nodes, ld, stride):
            key = (ptr, nodes, ld, stride)
            t = state["views"].get(key)
            if t is None:
                if len(state["views"]) > 256:
                    state["views"].clear()
                t = torch.as_tensor(_Panel(ptr, nodes, ld, stride), device=self.device)
                state["views"][key] = t
            return t

        def callback(_user, which, nodes, ld, _n, dX, xs, dY, ys, stream):
            t0 = time.perf_counter()
            try:
                X, Y = view(dX, nodes, ld, xs), view(dY, nodes, ld, ys)
                mul = muls[which]
                count(state, which)
                with torch.cuda.stream(torch.cuda.ExternalStream(stream or 0, device=self.device)):
                    if batched:
                        code = mul(Y, X)
                        code = int(code) if isinstance(code, int) else 0
                    else:
                        code = 0
                        for e in range(nodes):
                            ce = mul(Y[e], X[e])
                            if isinstance(ce, int) and ce != 0:
                                code = int(ce)
                                break
                return code
            except BaseException as exc:          # never let an exception cross the C frames
                state["error"] = exc
                return -1
            finally:
                state["callback_seconds"] += time.perf_counter() - t0

        return _lib.APPLY_FN(callback), state

    def set_term_operator(self, N, muls, *, real=True, symmetric=False, batched=False, norms=None, scratch_bytes=0):
        """Matrix-free split form (feasthip_set_term_operator): T(z) X = sum_k f_k(z) A_k X with ``muls[k](Y, X)`` writing A_k X
        into Y, or ``muls[k] = None`` for A_k = I (no call: the kernel reads X).  2 to 9 terms.  The views, ``real``, ``batched``,
        the stream rule and the failure rule are set_operator's; ``symmetric``: every A_k = A_k^T (what "cocg" needs, complex
        operators included).  The engine is then a term handle for the nep_* methods, poly_project_reduced and
        poly_orthonormalize, under set_solver("bicgstab" | "gmres" | "cocg") only.  ``norms``: set_term_norms.
        ``scratch_bytes``: bound of the product scratch (0: the library's default); when the nodes of a call do not fit, the
        callbacks see node chunks.  ``operator_stats()`` = {"term_calls": [per term], "callback_seconds"}."""
        N = int(N)
        muls = list(muls)
        if N < 1:
            raise ValueError("set_term_operator: N must be at least 1")
        if len(muls) < 2 or len(muls) > 9:
            raise ValueError(f"set_term_operator needs 2 to 9 terms, not {len(muls)}")
        if any(m is not None and not callable(m) for m in muls):
            raise ValueError("set_term_operator: each term must be callable, mul(Y, X) writes A_k X into Y, or None for the identity")
        if int(scratch_bytes) < 0:
            raise ValueError("set_term_operator: scratch_bytes must not be negative")

        def count(st, which):
            st["term_calls"][which] += 1

        cb, state = self._operator_thunk(N, muls, real, batched, {"term_calls": [0] * len(muls)}, count)
        flags = (0 if real else _lib.OP_COMPLEX) | (_lib.OP_SYMMETRIC if symmetric else 0)
        mask = sum(1 << k for k, m in enumerate(muls) if m is None)
        self._sync_stream()
        self._chk(self.lib.feasthip_set_term_operator(self.h, N, len(muls), cb, None, flags, mask, int(scratch_bytes)))
        self._op_thunk = cb
        self._op = state
        self.N, self.b_identity, self.poly_degree = N, False, len(muls) - 1
        self._problem_fp = None
        if norms is not None:
            self.set_term_norms(norms)

    def set_term_norms(self, norms):
        """nterms positive numbers that stand where ||A_k||_F stands in the backward errors of nep_ritz_eval on a term-operator
        handle (feasthip_set_term_norms)."""
        nv = np.ascontiguousarray(norms, dtype=np.float64)
        if nv.shape != (getattr(self, "poly_degree", 0) + 1,):
            raise ValueError("set_term_norms needs one norm per term")
        self._chk(self.lib.feasthip_set_term_norms(self.h, nv.ctypes.data_as(C.POINTER(C.c_double))))

    def operator_stats(self):
        """{A_calls, B_calls, callback_seconds} of the operator set by set_operator since it was set; for set_term_operator
        {"term_calls": [per term], "callback_seconds"}."""
        op = getattr(self, "_op", None)
        if op is None:
            return {"A_calls": 0, "B_calls": 0, "callback_seconds": 0.0}
        if "term_calls" in op:
            return {"term_calls": list(op["term_calls"]), "callback_seconds": op["callback_seconds"]}
        return {k: op[k] for k in ("A_calls", "B_calls", "callback_seconds")}

    def set_problem_csc(self, N, A_csc, B_csc=None, index_base=1):
        """Raw ``SparseMatrixCSC`` arrays (colptr, rowval, nzval) as the Julia shim passes them
        (set_matrices!): storage = CSC, 1-based by default; transposed on ingest."""
        pa, ia, va = A_csc
        cplx = np.iscomplexobj(va) or (B_csc is not None and np.iscomplexobj(B_csc[2]))
        dt = np.complex128 if cplx else np.float64
        pa, ia, va = np.ascontiguousarray(pa, dtype=np.int64), np.ascontiguousarray(ia, dtype=np.int64), np.ascontiguousarray(va, dtype=dt)
        if B_csc is not None:
            pb, ib, vb = (np.ascontiguousarray(B_csc[0], dtype=np.int64), np.ascontiguousarray(B_csc[1], dtype=np.int64),
                          np.ascontiguousarray(B_csc[2], dtype=dt))
            nb = len(vb)
        else:
            pb = ib = vb = None
            nb = 0
        self._chk(self.lib.feasthip_set_csr(self.h, int(N), int(cplx), int(index_base), 1, len(va), _np_ptr(pa), _np_ptr(ia), _np_ptr(va),
                                            nb, _np_ptr(pb), _np_ptr(ib), _np_ptr(vb)))
        self.N, self.b_identity = int(N), B_csc is None
        self._op = None
        self._problem_fp = None

    def set_contour(self, Zne, Wne, weight_scale):
        z = np.ascontiguousarray(Zne, dtype=np.complex128)
        w = np.ascontiguousarray(Wne, dtype=np.complex128)
        self._chk(self.lib.feasthip_set_contour(self.h, len(z), _np_ptr(z), _np_ptr(w), float(weight_scale)))
        self.ne = len(z)

    def set_real_projection(self, on):
        self._chk(self.lib.feasthip_set_real_projection(self.h, int(bool(on))))

    def set_adjoint(self, on):
        """While on, contour_apply, shifted_solve, matmul and ritz_residual act with the conjugate transposes
        (feasthip_set_adjoint): the solves reuse the LU factors the forward solves cached.  Dense problems with the
        direct solver, sparse problems with the sparse direct solver under its multifrontal plan or its blocked band LU
        (require_adjoint; the narrow one-workgroup band plan has no adjoint form), in fp64 only; persists on the engine."""
        self._chk(self.lib.feasthip_set_adjoint(self.h, int(bool(on))))

    def require_adjoint(self, on):
        """While on, the sparse direct solver plans for a CSR problem what has an adjoint substitution: the multifrontal
        LU, or -- where that plan does not exist for the pattern, or rejects a pivot -- the blocked band LU, never the
        narrow band plan (feasthip_require_adjoint): set before the first plan query or solve; persists on the engine."""
        self._chk(self.lib.feasthip_require_adjoint(self.h, int(bool(on))))

    def set_node_range(self, first, count):
        self._chk(self.lib.feasthip_set_node_range(self.h, int(first), int(count)))

    def set_node_list(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        self._chk(self.lib.feasthip_set_node_list(self.h, len(idx), _np_ptr(idx)))

    def set_solver(self, solver="direct", rtol=1e-12, atol=0.0, maxit=500, restart=30,
                   factor_precision=64, cache_factors=True):
        if solver not in _SOLVER_CODES:
            raise ValueError(f"Unsupported solver option '{solver}'. Use :direct, :banded, :bicgstab, :cocg, :shifted_cocg, :block_cocg, :gmres, or :iterative.")
        self._chk(self.lib.feasthip_set_solver(self.h, _SOLVER_CODES[solver], float(rtol), float(atol), int(maxit),
                                               int(restart), int(factor_precision), int(bool(cache_factors))))

    def set_node_solver(self, kinds):
        """Per-node solver (feasthip_set_node_solver): ``kinds[e]`` per GLOBAL contour node, 0 = the handle's solver,
        4 (``banded``) = a sparse direct solve for that node; ``None`` clears the setting."""
        if kinds is None:
            self._chk(self.lib.feasthip_set_node_solver(self.h, 0, None))
            return
        k = np.ascontiguousarray(kinds, dtype=np.int32)
        self._chk(self.lib.feasthip_set_node_solver(self.h, len(k), _np_ptr(k)))

    def set_preconditioner(self, pivots, node_pivot=None):
        """Shift preconditioner of the GMRES sweep (feasthip_set_preconditioner): ``pivots`` the complex pivot shifts (non-zero
        imaginary part), ``node_pivot[e]`` per GLOBAL contour node the index of its pivot, -1 = unpreconditioned.
        ``pivots=None`` (or empty) clears the setting."""
        if pivots is None or len(pivots) == 0:
            self._chk(self.lib.feasthip_set_preconditioner(self.h, 0, None, 0, None))
            return
        p = np.ascontiguousarray(pivots, dtype=np.complex128)
        k = np.ascontiguousarray(node_pivot, dtype=np.int32)
        self._chk(self.lib.feasthip_set_preconditioner(self.h, len(p), _np_ptr(p), len(k), _np_ptr(k)))

    def last_precond_sweep(self):
        """What the last sweep or shifted solve did under the preconditioner (feasthip_last_precond_sweep): a dict with
        used, pivots, factorizations, substitution_sweeps, factor_bytes and fell_back."""
        used, piv, fb = C.c_int(0), C.c_int(0), C.c_int(0)
        nf, sw, by = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.feasthip_last_precond_sweep(self.h, C.byref(used), C.byref(piv), C.byref(nf), C.byref(sw), C.byref(by),
                                                       C.byref(fb)))
        return {"used": bool(used.value), "pivots": piv.value, "factorizations": nf.value, "substitution_sweeps": sw.value,
                "factor_bytes": by.value, "fell_back": bool(fb.value)}

    # -- device arrays (plumbing) -----------------------------------------------------
    def set_column_mask(self, mask):
        """mask[c] == 0: column c is not iterated by the Krylov solvers (keeps its warm start);
        ``None`` clears the mask."""
        if mask is None:
            self._chk(self.lib.feasthip_set_column_mask(self.h, 0, None))
            return
        mk = np.ascontiguousarray(mask, dtype=np.int32)
        self._chk(self.lib.feasthip_set_column_mask(self.h, len(mk), _np_ptr(mk)))

    def empty(self, m):
        return self.torch.empty((m, self.N), dtype=self.torch.complex128, device=self.device)

    def upload(self, Q):
        """numpy N x m (any layout) -> device column-major block."""
        Qc = np.ascontiguousarray(np.asarray(Q, dtype=np.complex128).T)
        return self.torch.from_numpy(Qc).to(self.device)

    def download(self, dQ, m=None):
        a = dQ.cpu().numpy()
        if m is not None:
            a = a[:m]
        return np.asfortranarray(a.T)

    def _sync_stream(self):
        """Order the library behind torch.  torch's default stream has handle 0, for which
        the library falls back to its own non-blocking stream, so pending torch work (slice
        copies, the H2D/D2H halves of an all-reduce, NCCL kernels) is drained on the host
        first; every C-ABI call returns synchronised, which orders torch behind the library."""
        cur = self.torch.cuda.current_stream(self.device)
        cur.synchronize()
        if cur.cuda_stream != getattr(self, "_stream_handle", None):      # (set_stream drains the library's stream: only on a change)
            self._chk(self.lib.feasthip_set_stream(self.h, C.c_void_p(cur.cuda_stream)))
            self._stream_handle = cur.cuda_stream

    # -- hot path -------------------------------------------------------------------
    def contour_apply(self, dQ, m, ritz_lambda=None, want_moments=False):
        """Q_proj, per-node status, stats  [+ zAq, zSq].  With a communicator attached everything returned is
        already summed over the ranks (one packed RCCL all-reduce inside the call) and ``status`` is indexed by
        contour node; without one it is this handle's partial sum and ``status`` is per local node."""
        self._sync_stream()
        dP = self.empty(dQ.shape[0])
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        lam = None if ritz_lambda is None else np.ascontiguousarray(ritz_lambda, dtype=np.float64)
        dA = dS = None
        if want_moments:
            dA = self.torch.zeros((m, m), dtype=self.torch.complex128, device=self.device)
            dS = self.torch.zeros((m, m), dtype=self.torch.complex128, device=self.device)
        rc = self.lib.feasthip_contour_apply_dev(
            self.h, m, C.c_void_p(dQ.data_ptr()), _np_ptr(lam), C.c_void_p(dP.data_ptr()),
            C.c_void_p(dA.data_ptr()) if dA is not None else None,
            C.c_void_p(dS.data_ptr()) if dS is not None else None,
            _np_ptr(status), C.byref(stats))
        self._chk(rc)
        self.last_stats = stats.asdict()
        if want_moments:
            return dP, status, self.last_stats, dA.cpu().numpy().T.copy(), dS.cpu().numpy().T.copy()
        return dP, status, self.last_stats

    # -- stochastic eigenvalue-count estimate (fpm[14] = 2) -------------------------------------------------------------
    def random_block(self, m, seed):
        """The N x m Rademacher block (+-1, column-major device block: an (m, N) tensor) that estimate_count sweeps for
        ``seed`` (feasthip_random_block_dev)."""
        self._sync_stream()
        out = self.empty(int(m))
        self._chk(self.lib.feasthip_random_block_dev(self.h, int(m), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                     C.c_void_p(out.data_ptr())))
        return out

    def estimate_count(self, m, seed):
        """One contour sweep over m Rademacher columns and their Hutchinson samples t_j = v_j^T Q_proj[:, j]
        (feasthip_estimate_count) with the problem, contour, projection, solver and nodes set on the engine.
        Returns (samples: m complex values, status, stats); ``status`` as in contour_apply."""
        self._sync_stream()
        m = int(m)
        samples = np.zeros(2 * m, dtype=np.float64)
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        self._chk(self.lib.feasthip_estimate_count(self.h, m, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                   samples.ctypes.data_as(C.POINTER(C.c_double)), _np_ptr(status),
                                                   C.byref(stats)))
        self.last_stats = stats.asdict()
        return samples[0::2] + 1j * samples[1::2], status, self.last_stats

    # -- the refinement loop with resident panels (feasthip_*_resident: nothing crosses the ABI between the calls of a loop) --
    resident = True

    def contour_apply_resident(self, dQ, m, ritz_lambda=None):
        """The sweep of contour_apply with Q_proj left resident in the library.  dQ: device block to import, or None to
        sweep the Ritz vectors the last rr_ritz_resident left behind.  Returns (status, stats)."""
        self._sync_stream()
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        lam = None if ritz_lambda is None else np.ascontiguousarray(ritz_lambda, dtype=np.float64)
        self._chk(self.lib.feasthip_contour_apply_resident(self.h, int(m), C.c_void_p(dQ.data_ptr()) if dQ is not None else None,
                                                           _np_ptr(lam), _np_ptr(status), C.byref(stats)))
        self.last_stats = stats.asdict()
        return status, self.last_stats

    def rr_reduce_resident(self, m, rank_tol, hermitize=True):
        """rank of the resident Q_proj and the reduced pencil (Q_o^H A Q_o, Q_o^H B Q_o) of its orthonormal basis."""
        rank = C.c_int(0)
        Aq = np.zeros((m, m), dtype=np.complex128, order="F")
        Bq = np.zeros((m, m), dtype=np.complex128, order="F")
        self._chk(self.lib.feasthip_rr_reduce_resident(self.h, int(m), float(rank_tol), int(bool(hermitize)), C.byref(rank),
                                                       _np_ptr(Aq), _np_ptr(Bq)))
        r = int(rank.value)
        if r == m:
            return r, Aq, Bq
        # the library wrote r x r matrices contiguously
        return r, np.asfortranarray(Aq.ravel(order="F")[:r * r].reshape((r, r), order="F")), \
            np.asfortranarray(Bq.ravel(order="F")[:r * r].reshape((r, r), order="F"))

    def rr_ritz_resident(self, r, V, lam, M, normalize=True, use_B=True):
        """Ritz vectors X = Q_o V (left resident: the next sweep's subspace) and the residuals of the first M."""
        Vf = np.asfortranarray(V, dtype=np.complex128)
        lamc = np.ascontiguousarray(lam, dtype=np.complex128)
        res = np.zeros(max(1, r), dtype=np.float64)
        self._chk(self.lib.feasthip_rr_ritz_resident(self.h, int(r), _np_ptr(Vf), _np_ptr(lamc), int(M), int(normalize), int(use_B),
                                                     _np_ptr(res)))
        return res[:M].copy()

    def import_resident(self, dX, ncols, which=0):
        """A column-major device block becomes the resident subspace (which = 0) or the resident Q_proj (which = 1)."""
        self._sync_stream()
        self._chk(self.lib.feasthip_resident_import(self.h, int(which), int(ncols), C.c_void_p(dX.data_ptr())))

    def export_resident(self, ncols, which=0):
        """Column-major device block (ncols x N tensor) of the resident Ritz vectors (which = 0) or Q_proj (which = 1)."""
        out = self.torch.empty((max(int(ncols), 1), self.N), dtype=self.torch.complex128, device=self.device)
        self._chk(self.lib.feasthip_resident_export(self.h, int(which), int(ncols), C.c_void_p(out.data_ptr())))
        return out[:int(ncols)]

    ORTHO_METHODS = {"mgs": 0, "cholqr_rr": 1}
    ORTHO_USED = {0: "mgs", 1: "cholqr_rr", 2: "cholqr"}

    def set_ortho_method(self, method):
        """What a panel the Cholesky-QR fast path rejects takes: "mgs" (column-pivoted Gram-Schmidt, the default) or
        "cholqr_rr" (staged rank-revealing Cholesky-QR); feasthip_set_ortho_method.  Persists on the engine."""
        code = self.ORTHO_METHODS.get(method, method) if isinstance(method, str) else method
        if isinstance(code, str):
            raise ValueError(f"ortho must be one of {sorted(self.ORTHO_METHODS)}, not {method!r}")
        self._chk(self.lib.feasthip_set_ortho_method(self.h, int(code)))

    def last_ortho(self, n=0):
        """The last orthonormalisation (feasthip_last_ortho): method used ("cholqr" = the fast path), stages, fell_back, rank;
        with n > 0 also the first n entries of the pivot order and of |R_kk|."""
        used, stages, fell, rank = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        perm = np.full(max(1, n), -1, dtype=np.int32)
        rdiag = np.zeros(max(1, n), dtype=np.float64)
        self._chk(self.lib.feasthip_last_ortho(self.h, C.byref(used), C.byref(stages), C.byref(fell), C.byref(rank),
                                               _np_ptr(perm), _np_ptr(rdiag), int(n)))
        out = {"method": self.ORTHO_USED.get(used.value, used.value), "stages": stages.value, "fell_back": fell.value,
               "rank": rank.value}
        if n > 0:
            out["perm"], out["rdiag"] = perm[:n].copy(), rdiag[:n].copy()
        return out

    def orthonormalize(self, dQ, m, rank_tol):
        self._sync_stream()
        rank = C.c_int(0)
        self._chk(self.lib.feasthip_orthonormalize_dev(self.h, m, C.c_void_p(dQ.data_ptr()), float(rank_tol), C.byref(rank)))
        return rank.value

    def project(self, dQ, r, bilinear=False, hermitize=True):
        self._sync_stream()
        Aq = np.zeros((r, r), dtype=np.complex128, order="F")
        Bq = np.zeros((r, r), dtype=np.complex128, order="F")
        self._chk(self.lib.feasthip_project_dev(self.h, r, C.c_void_p(dQ.data_ptr()), int(bilinear), int(hermitize),
                                                _np_ptr(Aq), _np_ptr(Bq)))
        return Aq, Bq

    def project_pair(self, dQL, dQR, r):
        """The oblique reduced pencil of the two-sided method: (Q_L^H A Q_R, Q_L^H B Q_R), raw products
        (feasthip_project_pair_dev; Q_L^H Q_R for B = I)."""
        self._sync_stream()
        Aq = np.zeros((r, r), dtype=np.complex128, order="F")
        Bq = np.zeros((r, r), dtype=np.complex128, order="F")
        self._chk(self.lib.feasthip_project_pair_dev(self.h, r, C.c_void_p(dQL.data_ptr()), C.c_void_p(dQR.data_ptr()),
                                                     _np_ptr(Aq), _np_ptr(Bq)))
        return Aq, Bq

    def ritz_residual(self, dQ, r, V, lam, M, normalize=True, use_B=True):
        self._sync_stream()
        Vf = np.asfortranarray(V, dtype=np.complex128)
        lamc = np.ascontiguousarray(lam, dtype=np.complex128)
        dX = self.empty(dQ.shape[0])
        res = np.zeros(max(1, r), dtype=np.float64)
        self._chk(self.lib.feasthip_ritz_residual_dev(self.h, r, C.c_void_p(dQ.data_ptr()), _np_ptr(Vf), _np_ptr(lamc),
                                                      int(M), int(normalize), int(use_B), C.c_void_p(dX.data_ptr()),
                                                      _np_ptr(res)))
        return dX, res[:M].copy()

    def rayleigh_ritz(self, dQ, r, Emin, Emax, use_B=True):
        """Project, solve the reduced Hermitian-definite pencil ON THE DEVICE (Jacobi), reorder inside-first,
        back-transform and measure residuals in one call.  Returns (dX, lambda[r], M, res[M]), or None when
        the reduced B matrix is not positive definite (caller falls back to the host eigensolver)."""
        self._sync_stream()
        dX = self.empty(dQ.shape[0])
        lam = np.zeros(r, dtype=np.float64)
        res = np.zeros(r, dtype=np.float64)
        M = C.c_int(0)
        rc = self.lib.feasthip_rayleigh_ritz_dev(self.h, r, C.c_void_p(dQ.data_ptr()), float(Emin), float(Emax), int(bool(use_B)),
                                                 C.c_void_p(dX.data_ptr()), _np_ptr(lam), C.byref(M), _np_ptr(res))
        if rc == 8:
            return None
        self._chk(rc)
        return dX, lam, int(M.value), res[:int(M.value)]

    def matmul(self, which, dX, m):
        self._sync_stream()
        dY = self.empty(dX.shape[0])
        self._chk(self.lib.feasthip_matmul_dev(self.h, int(which), m, C.c_void_p(dX.data_ptr()), C.c_void_p(dY.data_ptr())))
        return dY

    def shifted_solve(self, z, dX, m):
        self._sync_stream()
        dY = self.empty(dX.shape[0])
        stats = FeastHipStats()
        rc = self.lib.feasthip_shifted_solve_dev(self.h, float(np.real(z)), float(np.imag(z)), m,
                                                 C.c_void_p(dX.data_ptr()), C.c_void_p(dY.data_ptr()), C.byref(stats))
        self._chk(rc, ok=(0, 5, 8))
        self.last_stats = stats.asdict()
        return dY, rc

    # -- polynomial eigenproblems (feasthip_poly_*): linearised blocks are column-major dN x m, i.e. (m, d N) tensors ------------
    def set_polynomial(self, coeffs, terms=False):
        """P(lambda) = sum_k lambda^k coeffs[k] becomes the engine's problem (feasthip_set_polynomial): dense square matrices
        of one size, real or complex; afterwards only the poly_* methods, set_contour, set_solver("direct") and free_factors
        apply until set_problem installs a pencil again.  ``terms``: the matrices are the A_k of a split form instead
        (set_terms)."""
        mats = [np.asarray(c) for c in coeffs]
        if len(mats) < 2:
            raise ValueError("a split form needs at least two terms" if terms else "a polynomial needs at least two coefficient matrices")
        N = mats[0].shape[0]
        for c in mats:
            if c.ndim != 2 or c.shape != (N, N):
                raise ValueError("coefficient matrices must be square and of one size")
        cplx = any(np.iscomplexobj(c) for c in mats)
        dt = np.complex128 if cplx else np.float64
        fs = [np.asfortranarray(c, dtype=dt) for c in mats]
        ptrs = (C.c_void_p * len(fs))(*[f.ctypes.data for f in fs])
        lds = np.full(len(fs), N, dtype=np.int64)
        if terms:
            self._chk(self.lib.feasthip_set_terms(self.h, N, len(fs), int(cplx), ptrs, _np_ptr(lds)))
        else:
            self._chk(self.lib.feasthip_set_polynomial(self.h, N, len(fs) - 1, int(cplx), ptrs, _np_ptr(lds)))
        self.N, self.b_identity, self.poly_degree = N, False, len(fs) - 1
        self._op = None
        self._problem_fp = None

    def set_polynomial_csr(self, rowptr, col, vals, terms=False):
        """The same for sparse coefficients on one CSR pattern (feasthip_set_polynomial_csr; ingest.polynomial_union_csr makes
        the arrays): rowptr / col 0-based, vals[k] the values of coeffs[k] on the pattern.  The poly_* methods work as on a
        dense polynomial; P(z_e) is factored by the multifrontal LU of the sparse direct solver (band_plan, direct_plan_flops
        and direct_plan_bytes describe it), or, after set_solver("bicgstab" | "cocg" | "gmres"), poly_solve and poly_resinv_apply
        solve with that Krylov method on the operator P(z_e) and nothing is factored.  ``terms``: set_terms_csr."""
        if len(vals) < 2:
            raise ValueError("a split form needs at least two terms" if terms else "a polynomial needs at least two coefficient matrices")
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        cl = np.ascontiguousarray(col, dtype=np.int64)
        N = len(rp) - 1
        cplx = any(np.iscomplexobj(v) for v in vals)
        vs = [np.ascontiguousarray(v, dtype=np.complex128 if cplx else np.float64) for v in vals]
        if N < 1 or rp[-1] != len(cl) or any(v.shape != (len(cl),) for v in vs):
            raise ValueError("rowptr, col and the value arrays do not describe one pattern")
        ptrs = (C.c_void_p * len(vs))(*[v.ctypes.data for v in vs])
        if terms:
            self._chk(self.lib.feasthip_set_terms_csr(self.h, N, len(vs), int(cplx), _np_ptr(rp), _np_ptr(cl), ptrs))
        else:
            self._chk(self.lib.feasthip_set_polynomial_csr(self.h, N, len(vs) - 1, int(cplx), _np_ptr(rp), _np_ptr(cl), ptrs))
        self.N, self.b_identity, self.poly_degree = N, False, len(vs) - 1
        self._op = None
        self._problem_fp = None

    def _poly_empty(self, m):
        return self.torch.empty((m, self.poly_degree * self.N), dtype=self.torch.complex128, device=self.device)

    def poly_solve(self, z, dR, m):
        """Y = P(z)^-1 R on an N x m device block -> (dY, code 0 | 8); feasthip_poly_solve_dev.  Under a Krylov solver (sparse
        coefficients) the code is 0 or 5 (a column stopped at maxit) and last_stats holds the iteration counts."""
        self._sync_stream()
        dY = self.empty(dR.shape[0])
        stats = FeastHipStats()
        rc = self.lib.feasthip_poly_solve_dev(self.h, float(np.real(z)), float(np.imag(z)), int(m), C.c_void_p(dR.data_ptr()),
                                              C.c_void_p(dY.data_ptr()), C.byref(stats))
        self._chk(rc, ok=(0, 5, 8))
        self.last_stats = stats.asdict()
        return dY, rc

    def poly_contour_apply(self, dQ, m):
        """Q_proj = sum_e w_e (z_e B_lin - A_lin)^-1 B_lin Q on a dN x m device block -> (dP, status per node, stats)."""
        self._sync_stream()
        dP = self._poly_empty(dQ.shape[0])
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        self._chk(self.lib.feasthip_poly_contour_apply_dev(self.h, int(m), C.c_void_p(dQ.data_ptr()), C.c_void_p(dP.data_ptr()),
                                                           _np_ptr(status), C.byref(stats)))
        self.last_stats = stats.asdict()
        return dP, status, self.last_stats

    def poly_matmul(self, which, dX, m):
        """A_lin X (which 0) or B_lin X (which 1) on a dN x m device block."""
        self._sync_stream()
        dY = self._poly_empty(dX.shape[0])
        self._chk(self.lib.feasthip_poly_matmul_dev(self.h, int(which), int(m), C.c_void_p(dX.data_ptr()), C.c_void_p(dY.data_ptr())))
        return dY

    def poly_node_products(self, dX, m, dB=None):
        """The operator of the Krylov solvers as a product (sparse coefficients, m <= 64): dX holds one N x m block per contour
        node, an (ne m, N) tensor -> the same shape with Y_e = P(z_e) X_e, or Y_e = B - P(z_e) X_e for dB an (m, N) tensor
        shared by the nodes, or Y_e = B_e - P(z_e) X_e for dB of dX's shape (feasthip_poly_matmul_dev, which 2 | 3 | 4)."""
        m = int(m)
        if dX.shape[0] != self.ne * m:
            raise ValueError("poly_node_products needs one N x m block per contour node")
        which = 2
        dY = self.empty(dX.shape[0])
        if dB is not None:
            if dB.shape[0] not in (m, self.ne * m):
                raise ValueError("poly_node_products: B is one N x m block, or one per node")
            which = 3 if dB.shape[0] == m else 4
            dY[:dB.shape[0]].copy_(dB)
        self._sync_stream()
        self._chk(self.lib.feasthip_poly_matmul_dev(self.h, which, m, C.c_void_p(dX.data_ptr()), C.c_void_p(dY.data_ptr())))
        return dY

    def poly_project(self, dQ, r):
        """(Q^H A_lin Q, Q^H B_lin Q), raw products, r x r on the host."""
        self._sync_stream()
        Aq = np.zeros((r, r), dtype=np.complex128, order="F")
        Sq = np.zeros((r, r), dtype=np.complex128, order="F")
        self._chk(self.lib.feasthip_poly_project_dev(self.h, int(r), C.c_void_p(dQ.data_ptr()), _np_ptr(Aq), _np_ptr(Sq)))
        return Aq, Sq

    def poly_ritz_residual(self, dQ, r, V, lam, M, normalize=True, use_B=True):
        """X = Q V on the linearisation, the first M columns normalised -> (dX, res[M], backward_error[M]): the linearised
        residual with (use_B) or without B_lin, and the backward error of (lambda_j, first block of x_j) in P."""
        self._sync_stream()
        Vf = np.asfortranarray(V, dtype=np.complex128)
        lamc = np.ascontiguousarray(lam, dtype=np.complex128)
        dX = self._poly_empty(dQ.shape[0])
        res = np.zeros(max(1, r), dtype=np.float64)
        bwd = np.zeros(max(1, r), dtype=np.float64)
        self._chk(self.lib.feasthip_poly_ritz_residual_dev(self.h, int(r), C.c_void_p(dQ.data_ptr()), _np_ptr(Vf), _np_ptr(lamc),
                                                           int(M), int(normalize), int(use_B), C.c_void_p(dX.data_ptr()),
                                                           _np_ptr(res), _np_ptr(bwd)))
        return dX, res[:M].copy(), bwd[:M].copy()

    # -- projected method: N x m blocks, i.e. (m, N) tensors as for a pencil -------------------------------------------------------
    def poly_eval_cols(self, dX, lam, m):
        """R[:, j] = P(lam_j) X[:, j] on an N x m device block (feasthip_poly_eval_cols_dev)."""
        self._sync_stream()
        lamc = np.ascontiguousarray(lam, dtype=np.complex128)
        if lamc.shape != (int(m),):
            raise ValueError("poly_eval_cols needs one value per column")
        dR = self.empty(dX.shape[0])
        self._chk(self.lib.feasthip_poly_eval_cols_dev(self.h, int(m), _np_ptr(lamc), C.c_void_p(dX.data_ptr()), C.c_void_p(dR.data_ptr())))
        return dR

    def poly_resinv_apply(self, dX, m, sigma=None):
        """The projected method's contour step on an N x m device block -> (dQ, status per node, stats): the plain sweep
        sum_e w_e P(z_e)^-1 X (sigma None), else the residual-inverse sweep with one shift per column
        (feasthip_poly_resinv_apply_dev).  Under a Krylov solver a node's status is 0 or 5 (a column stopped at maxit)."""
        self._sync_stream()
        sg = None
        if sigma is not None:
            sg = np.ascontiguousarray(sigma, dtype=np.complex128)
            if sg.shape != (int(m),):
                raise ValueError("poly_resinv_apply needs one shift per column")
        dQ = self.empty(dX.shape[0])
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        self._chk(self.lib.feasthip_poly_resinv_apply_dev(self.h, int(m), None if sg is None else _np_ptr(sg), C.c_void_p(dX.data_ptr()),
                                                          C.c_void_p(dQ.data_ptr()), _np_ptr(status), C.byref(stats)))
        self.last_stats = stats.asdict()
        return dQ, status, self.last_stats

    def poly_project_reduced(self, dQ, r):
        """[Q^H A_k Q for k = 0 .. d], r x r on the host (feasthip_poly_project_reduced_dev)."""
        self._sync_stream()
        d = getattr(self, "poly_degree", 1)
        Ahat = np.zeros((d + 1, r, r), dtype=np.complex128)       # [k] column-major r x r == [k].T in C order
        self._chk(self.lib.feasthip_poly_project_reduced_dev(self.h, int(r), C.c_void_p(dQ.data_ptr()), _np_ptr(Ahat)))
        return [np.asfortranarray(Ahat[k].T) for k in range(d + 1)]

    def poly_ritz_eval(self, dQ, r, Y, theta=None):
        """X = Q Y with unit columns (Y: r x ncand) -> (dX, backward_error[ncand] of the pairs (theta_i, x_i), or None without
        theta); feasthip_poly_ritz_eval_dev."""
        self._sync_stream()
        Yf = np.asfortranarray(Y, dtype=np.complex128)
        ncand = Yf.shape[1]
        if Yf.shape[0] != int(r):
            raise ValueError("poly_ritz_eval: Y must have r rows")
        dX = self.empty(ncand)
        th = bwd = None
        if theta is not None:
            th = np.ascontiguousarray(theta, dtype=np.complex128)
            if th.shape != (ncand,):
                raise ValueError("poly_ritz_eval needs one value per candidate")
            bwd = np.zeros(ncand, dtype=np.float64)
        self._chk(self.lib.feasthip_poly_ritz_eval_dev(self.h, int(r), C.c_void_p(dQ.data_ptr()), int(ncand), _np_ptr(Yf),
                                                       None if th is None else _np_ptr(th), C.c_void_p(dX.data_ptr()),
                                                       None if bwd is None else _np_ptr(bwd)))
        return dX, bwd

    def poly_orthonormalize(self, dQ, m, rank_tol, unit_columns=True):
        """Rank-revealing orthonormalisation of the N x m block of a polynomial handle, in place -> rank
        (feasthip_poly_orthonormalize_dev; set_ortho_method and last_ortho apply as for a pencil)."""
        self._sync_stream()
        rank = C.c_int(0)
        self._chk(self.lib.feasthip_poly_orthonormalize_dev(self.h, int(m), C.c_void_p(dQ.data_ptr()), int(bool(unit_columns)),
                                                            float(rank_tol), C.byref(rank)))
        return rank.value

    # -- nonlinear eigenproblems in split form (feasthip_nep_*): a term handle, the scalars f_k(.) as host tables --------------------
    def set_terms(self, mats):
        """T(lambda) = sum_k f_k(lambda) mats[k] becomes the engine's problem (feasthip_set_terms): a term handle.  The f_k stay
        with the caller; the nep_* methods take tables of their values, poly_project_reduced and poly_orthonormalize work as on
        a polynomial, every other poly_* method is refused."""
        self.set_polynomial(mats, terms=True)

    def set_terms_csr(self, rowptr, col, vals):
        """The same for sparse terms on one CSR pattern (feasthip_set_terms_csr; ingest.polynomial_union_csr makes the arrays)."""
        self.set_polynomial_csr(rowptr, col, vals, terms=True)

    def _nep_table(self, F, rows, what):
        Fc = np.ascontiguousarray(F, dtype=np.complex128)
        if Fc.shape != (int(rows), self.poly_degree + 1):
            raise ValueError(f"{what} needs a table of shape ({int(rows)}, {self.poly_degree + 1})")
        return Fc

    def nep_set_node_values(self, F):
        """F[e, k] = f_k(z_e) on the contour of the last set_contour (feasthip_nep_set_node_values)."""
        Fc = np.ascontiguousarray(F, dtype=np.complex128)
        if Fc.ndim != 2 or Fc.shape[1] != self.poly_degree + 1:
            raise ValueError("nep_set_node_values needs one row of nterms values per contour node")
        self._chk(self.lib.feasthip_nep_set_node_values(self.h, Fc.shape[0], _np_ptr(Fc)))

    def nep_solve(self, node, dR, m):
        """Y = T(z_node)^-1 R on an N x m device block -> (dY, code 0 | 8); feasthip_nep_solve_dev.  On a term-operator handle
        (a Krylov solve) the code is 0 or 5 (a column stopped at maxit) and last_stats holds the iteration counts."""
        self._sync_stream()
        dY = self.empty(dR.shape[0])
        stats = FeastHipStats()
        rc = self.lib.feasthip_nep_solve_dev(self.h, int(node), int(m), C.c_void_p(dR.data_ptr()), C.c_void_p(dY.data_ptr()), C.byref(stats))
        self._chk(rc, ok=(0, 5, 8))
        self.last_stats = stats.asdict()
        return dY, rc

    def nep_eval_cols(self, dX, F, m):
        """R[:, j] = sum_k F[j, k] A_k X[:, j] on an N x m device block (feasthip_nep_eval_cols_dev)."""
        self._sync_stream()
        Fc = self._nep_table(F, m, "nep_eval_cols")
        dR = self.empty(dX.shape[0])
        self._chk(self.lib.feasthip_nep_eval_cols_dev(self.h, int(m), _np_ptr(Fc), C.c_void_p(dX.data_ptr()), C.c_void_p(dR.data_ptr())))
        return dR

    def nep_resinv_apply(self, dX, m, sigma=None, F_sigma=None):
        """The contour step on an N x m device block of a term handle -> (dQ, status per node, stats): the plain sweep (sigma
        and F_sigma None), else the residual-inverse sweep with F_sigma[j, k] = f_k(sigma_j) (feasthip_nep_resinv_apply_dev)."""
        self._sync_stream()
        sg = Fc = None
        if sigma is not None:
            sg = np.ascontiguousarray(sigma, dtype=np.complex128)
            if sg.shape != (int(m),):
                raise ValueError("nep_resinv_apply needs one shift per column")
        if F_sigma is not None:
            Fc = self._nep_table(F_sigma, m, "nep_resinv_apply")
        dQ = self.empty(dX.shape[0])
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        self._chk(self.lib.feasthip_nep_resinv_apply_dev(self.h, int(m), None if sg is None else _np_ptr(sg), None if Fc is None else _np_ptr(Fc),
                                                         C.c_void_p(dX.data_ptr()), C.c_void_p(dQ.data_ptr()), _np_ptr(status), C.byref(stats)))
        self.last_stats = stats.asdict()
        return dQ, status, self.last_stats

    def nep_ritz_eval(self, dQ, r, Y, F_theta=None):
        """X = Q Y with unit columns (Y: r x ncand) -> (dX, backward_error[ncand] of the pairs (theta_i, x_i) from F_theta[i, k]
        = f_k(theta_i), or None without the table); feasthip_nep_ritz_eval_dev."""
        self._sync_stream()
        Yf = np.asfortranarray(Y, dtype=np.complex128)
        ncand = Yf.shape[1]
        if Yf.shape[0] != int(r):
            raise ValueError("nep_ritz_eval: Y must have r rows")
        dX = self.empty(ncand)
        Fc = bwd = None
        if F_theta is not None:
            Fc = self._nep_table(F_theta, ncand, "nep_ritz_eval")
            bwd = np.zeros(ncand, dtype=np.float64)
        self._chk(self.lib.feasthip_nep_ritz_eval_dev(self.h, int(r), C.c_void_p(dQ.data_ptr()), int(ncand), _np_ptr(Yf),
                                                      None if Fc is None else _np_ptr(Fc), C.c_void_p(dX.data_ptr()),
                                                      None if bwd is None else _np_ptr(bwd)))
        return dX, bwd

    def poly_estimate_count(self, m, seed, G, want_block=False):
        """Hutchinson samples of the eigenvalue count of a polynomial or term handle (feasthip_poly_estimate_count):
        t_c = v_c^T [sum_e w_e T'(z_e) T(z_e)^-1 v_c] for the m Rademacher columns of ``seed``, with G[e, k] = w_e g_k(z_e) the
        ne x (degree + 1) table of T'(z_e) = sum_k g_k(z_e) A_k (hip_backend.poly_derivative_table / nep_derivative_table times
        the weights).  Returns (samples: m complex values, status per node, stats), and with ``want_block`` also the block V the
        samples were taken with (an (m, N) tensor)."""
        self._sync_stream()
        m = int(m)
        Gc = np.ascontiguousarray(G, dtype=np.complex128)
        if Gc.shape != (max(1, self.ne), self.poly_degree + 1):
            raise ValueError(f"poly_estimate_count needs a table of shape ({self.ne}, {self.poly_degree + 1})")
        samples = np.zeros(2 * max(m, 0), dtype=np.float64)
        status = np.zeros(max(1, self.ne), dtype=np.int32)
        stats = FeastHipStats()
        dV = self.empty(m) if want_block and m > 0 else None
        self._chk(self.lib.feasthip_poly_estimate_count(self.h, m, C.c_uint64(int(seed) & (2 ** 64 - 1)), _np_ptr(Gc),
                                                        samples.ctypes.data_as(C.POINTER(C.c_double)),
                                                        None if dV is None else C.c_void_p(dV.data_ptr()), _np_ptr(status),
                                                        C.byref(stats)))
        self.last_stats = stats.asdict()
        t = samples[0::2] + 1j * samples[1::2]
        return (t, status, self.last_stats, dV) if want_block else (t, status, self.last_stats)

    def free_factors(self):
        """Drop the cached LU / band factors of the direct solvers (feasthip_release_factors)."""
        self._chk(self.lib.feasthip_release_factors(self.h))

    # `blocked` of band_plan(): the plan of the sparse direct solver
    PLAN_NARROW, PLAN_BAND, PLAN_MULTIFRONTAL = 0, 1, 2

    def band_plan(self):
        """(kl, ku, bytes per node, blocked) of the band the direct sparse solver would eliminate (feasthip_band_plan)."""
        kl, ku, blocked = C.c_int(0), C.c_int(0), C.c_int(0)
        nbytes = C.c_int64(0)
        self._chk(self.lib.feasthip_band_plan(self.h, C.byref(kl), C.byref(ku), C.byref(nbytes), C.byref(blocked)))
        return kl.value, ku.value, nbytes.value, blocked.value

    def direct_plan_flops(self):
        """real flops of one node's factorisation under the direct solver's plan (band LU or multifrontal)."""
        fl = C.c_double(0.0)
        self._chk(self.lib.feasthip_direct_plan_flops(self.h, C.byref(fl)))
        return fl.value

    def direct_plan_bytes(self, nodes):
        """(factor bytes, transient bytes) that ``nodes`` direct nodes take on the device (feasthip_direct_plan_bytes)."""
        fb, tb = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.feasthip_direct_plan_bytes(self.h, int(nodes), C.byref(fb), C.byref(tb)))
        return fb.value, tb.value

    def last_node_iterations(self, n):
        out = np.zeros(max(1, n), dtype=np.int32)
        self._chk(self.lib.feasthip_last_node_iterations(self.h, _np_ptr(out), int(n)))
        return out[:n]

    def last_shifted_sweep(self):
        """(used, seed node, seed iterations, SpMM node-passes) of the last contour_apply: whether it took the shifted COCG
        sweep (solver "shifted_cocg" on an eligible problem) and what that cost (feasthip_last_shifted_sweep)."""
        out = [np.zeros(1, dtype=np.int32) for _ in range(4)]
        self._chk(self.lib.feasthip_last_shifted_sweep(self.h, *[_np_ptr(v) for v in out]))
        return bool(out[0][0]), int(out[1][0]), int(out[2][0]), int(out[3][0])

    def last_block_sweep(self):
        """(used, most block steps of a node, nodes that broke down, SpMM node-passes) of the last contour_apply: whether it
        took the block COCG sweep (solver "block_cocg" on an eligible problem) and what that cost
        (feasthip_last_block_sweep)."""
        out = [np.zeros(1, dtype=np.int32) for _ in range(4)]
        self._chk(self.lib.feasthip_last_block_sweep(self.h, *[_np_ptr(v) for v in out]))
        return bool(out[0][0]), int(out[1][0]), int(out[2][0]), int(out[3][0])

    def last_global_node_iterations(self):
        """Per contour node, summed over the ranks (multi-rank sweeps only): the cost signal for node re-balancing."""
        out = np.zeros(max(1, self.ne), dtype=np.int32)
        self._chk(self.lib.feasthip_last_global_node_iterations(self.h, _np_ptr(out), int(self.ne)))
        return out[:self.ne]

    def last_column_iterations(self, nodes, m):
        out = np.zeros(max(1, nodes * m), dtype=np.int32)
        self._chk(self.lib.feasthip_last_column_iterations(self.h, _np_ptr(out), int(nodes * m)))
        return out[:nodes * m].reshape(nodes, m)

    # -- measurement ----------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self.lib.feasthip_profile_enable(self.h, int(on)))

    def profile_set_period(self, period):
        self._chk(self.lib.feasthip_profile_set_period(self.h, int(period)))

    def profile_get_work(self, cls):
        w = C.c_double(0)
        self._chk(self.lib.feasthip_profile_get_work(self.h, cls.encode(), C.byref(w)))
        return w.value

    def profile_reset(self):
        self._chk(self.lib.feasthip_profile_reset(self.h))

    def profile_get(self, cls):
        ms, n = C.c_double(0), C.c_int64(0)
        self._chk(self.lib.feasthip_profile_get(self.h, cls.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def synchronize(self):
        self._chk(self.lib.feasthip_synchronize(self.h))
