"""What the Python wrappers of dla_future_amd pass across the C ABI, recorded without the library and without a GPU.

A recording stand-in is assigned to ``dla_future_amd.capi._lib``, so ``lib()`` returns it and nothing is loaded.  For
every name in ``capi.SIGNATURES`` the stand-in gives a callable that appends ``(name, normalised arguments)`` to a log
and returns a fixed value (0 for c_int, 2 for c_long, 0.5 for float / double).  ``CASES`` drives every public name that
reaches the library at tiny sizes.  Each case runs twice: with every c_int entry returning 0, and with every c_int entry
returning 7; the second run records the type and the message of the exception the wrapper raises, or the value it
returns.  ``signatures()`` gives a text of (restype, argtypes) of every key of ``SIGNATURES``.

``python tests/abi_call_cases.py OUT.json`` writes the sections.  tests/golden/python_abi_calls.json is that output AT
THE COMMIT BEFORE the binding was split into modules (this file was copied into a checkout of it): it pins the behaviour
the split had to keep.  It is NEVER regenerated from refactored code -- a difference is a change of what crosses the ABI
and is to be judged as such; only a new entry point adds entries, recorded by the commit that adds it.

The file is kept small, so everything is a short text.  An entry of "calls" is [the calls, the outcome when every entry
succeeds, the outcome when c_int entries return 7 (, the number of calls made then, where it differs)].  A call is
"name(arg,...)" with "~" for the prefix dlaf_mi355x_: ints and floats as they are; bytes quoted (hex after "x" when not
printable, "+0*n" for n trailing zeros); a Structure as Name(fields); a ctypes array as [..]; byref(x) as "&type(value)";
a c_void_p as "-" (NULL), as the case's name of the numpy array it points to (by address), as "#k" for the k-th opaque
handle created in the case, and else as the bytes at it ("x" + hex, "0*n" when all n are 0), read with the length the
case declares for that argument position (never more).  An outcome is "= value" (an array as dtype[shape]F/C=0 when all
zero, else a digest) or "! Exception: message", where "$k" stands for the name of the case's k-th call.  Types: i l c p
d f are c_int, c_long, c_char, c_void_p, c_double, c_float, "*t" a POINTER, "FN(res;args)" a CFUNCTYPE, D DLAFDescriptor;
a Structure is given by name in "signatures" and with its (field, type) list in "structures".
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, NB, NRHS = 8, 4, 3
DT = {"s": np.dtype(np.float32), "d": np.dtype(np.float64), "c": np.dtype(np.complex64), "z": np.dtype(np.complex128)}
RT = {"s": DT["s"], "d": DT["d"], "c": DT["s"], "z": DT["d"]}
T4 = "sdcz"
OPAQUE = "opaque"  # a pointer whose target holds nothing stable (uninitialised memory, a code address)


class HarnessError(Exception):
    """The case table does not describe a call (never caught by a case)."""


# one letter for the common types, so that the recorded file stays small; every other type by its ctypes name
SHORT = {C.c_int: "i", C.c_long: "l", C.c_char: "c", C.c_void_p: "p", C.c_double: "d", C.c_float: "f"}
PREFIX = "dlaf_mi355x_"  # written "~" in the recorded calls


def _type_text(t):
    if t is None:
        return "void"
    if t in SHORT:
        return SHORT[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "*" + _type_text(t._type_)
    if isinstance(t, type) and issubclass(t, C._CFuncPtr):
        return f"FN({_type_text(t._restype_)};{','.join(_type_text(x) for x in t._argtypes_)})"
    return "D" if t.__name__ == "DLAFDescriptor" else t.__name__  # (a Structure by name: its fields are under "structures")


def signatures(capi):
    return {name: f"{_type_text(res)}({','.join(_type_text(x) for x in args)})"
            for name, (res, args) in capi.SIGNATURES.items()}


def structures(capi):
    """The (field, type) list of every Structure that capi defines."""
    return {_type_text(v): ",".join(f"{n}:{_type_text(x)}" for n, x in v._fields_) for k, v in vars(capi).items()
            if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def _fields(s):
    return f"{_type_text(type(s))}({','.join(str(getattr(s, f)) for f, _ in s._fields_)})"


class Recorder:
    def __init__(self, capi):
        self._sig = capi.SIGNATURES
        self._log, self._arrays, self._scal, self._handles, self._ret = None, {}, {}, [], 0

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._sig:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        if self._log is not None:
            self._log.append(f"{name}({','.join(self._norm(name, i, a) for i, a in enumerate(args))})".replace(PREFIX, "~", 1))
        res = self._sig[name][0]
        if res is C.c_int:
            if self._ret == 0 and name in ("dlaf_mi355x_matrix_create", "dlaf_mi355x_gmatrix_create"):
                args[-1]._obj.value = 0x1000 * (len(self._handles) + 1)
                self._handles.append(args[-1]._obj.value)
            return self._ret
        if res is None:
            return None
        if res is C.c_long:
            return 2
        if res in (C.c_float, C.c_double):
            return 0.5
        if res is C.c_char_p:
            return b"stand-in"
        raise HarnessError(f"{name}: no stand-in value for {res}")

    def _norm(self, name, i, a):
        if a is None:
            return "-"
        if type(a) in (bool, int, float):
            return repr(a)
        if type(a) is bytes:
            return _bytes(a)
        if isinstance(a, (np.integer, np.floating)):
            return f"{type(a).__name__}:{a!r}"
        if isinstance(a, C.Structure):
            return _fields(a)
        if isinstance(a, C.Array):
            if a._type_ is C.c_char:
                return _bytes(a.raw)
            return "[" + ",".join(self._norm(name, i, x) for x in a) + "]"
        if isinstance(a, C._CFuncPtr):
            return _type_text(type(a))
        if type(a).__name__ == "CArgObject":
            o = a._obj
            return "&" + (_fields(o) if isinstance(o, C.Structure) else f"{_type_text(type(o))}({o.value})")
        if isinstance(a, C.c_void_p):
            v = a.value
            if v is None:
                return "-"
            if v in self._handles:
                return f"#{self._handles.index(v)}"
            for key, arr in self._arrays.items():
                if arr.size and arr.ctypes.data == v:
                    return key
            n = self._scal.get(i)
            if n == OPAQUE:
                return OPAQUE
            if n is None:
                raise HarnessError(f"{name}: argument {i} points to nothing the case declares")
            raw = C.string_at(v, n)
            return f"0*{n}" if not any(raw) else "x" + raw.hex()
        raise HarnessError(f"{name}: argument {i} of type {type(a)}")

    @contextlib.contextmanager
    def _quiet(self):
        """fixtures are built with the log off and every entry succeeding"""
        saved = self._log, self._ret
        self._log, self._ret = None, 0
        try:
            yield
        finally:
            self._log, self._ret = saved


class Fixtures:
    """Per case: named arrays, grids and resident matrices (built quietly)."""

    def __init__(self, rec, daf):
        self.rec, self.daf, self.arrays, self._keep = rec, daf, {}, []

    def arr(self, name, shape, dtype):
        shape = (shape,) if isinstance(shape, int) else shape
        a = np.asfortranarray((np.arange(int(np.prod(shape))) % 7 + 1).reshape(shape, order="F").astype(dtype))
        self.arrays[name] = a
        return a

    def g1(self):
        with self.rec._quiet():
            return self.daf.Grid.single()

    def g4(self):
        with self.rec._quiet():
            return self.daf.Grid.rccl(b"id", 4, 1, 2, 2)

    def dm(self, t, uplo="L"):
        with self.rec._quiet():
            m = self.daf.DeviceMatrix(self.daf.Grid.single(), DT[t], uplo, N, NB)
        self._keep.append(m)
        return m

    def gm(self, t, m=N, n=NRHS):
        with self.rec._quiet():
            g = self.daf.GeneralDeviceMatrix(self.daf.Grid.single(), DT[t], m, n, NB)
        self._keep.append(g)
        return g

    def close(self):
        with self.rec._quiet():
            for m in self._keep:
                m.close()


def _bytes(b: bytes) -> str:
    """printable bytes quoted, trailing zeros counted"""
    body = b.rstrip(b"\0")
    text = repr(body)[1:] if all(32 <= c < 127 for c in body) else "x" + body.hex()
    return text + (f"+0*{len(b) - len(body)}" if len(b) > len(body) else "")


def _result(x) -> str:
    """What a wrapper returned, as a short text: an array as dtype[shape], F or C, and 0 (all zeros) or a digest."""
    if x is None or type(x) in (bool, int, float, str):
        return repr(x)
    if isinstance(x, bytes):
        return _bytes(x)
    if isinstance(x, (np.integer, np.floating)):
        return f"{type(x).__name__}:{x!r}"
    if isinstance(x, np.ndarray):
        what = "0" if not x.any() else hashlib.sha1(x.tobytes(order="F")).hexdigest()[:8]
        return f"{x.dtype}{list(x.shape)}{'F' if x.flags.f_contiguous else 'C'}={what}"
    if isinstance(x, (tuple, list)):
        return "(" + ",".join(_result(y) for y in x) + ")"
    if isinstance(x, dict):
        return "{" + ",".join(f"{k}:{_result(v)}" for k, v in x.items()) + "}"
    attrs = ",".join(f"{k}={v!r}" for k, v in sorted(vars(x).items()) if type(v) in (bool, int, float, str))
    return f"{type(x).__name__}<{attrs}>"


# ---- the case table: (id, callable(K: Fixtures), {argument position: bytes of the boxed value there}) ---------------
CASES = []


def case(cid, fn, scal=None):
    CASES.append((cid, fn, scal or {}))


def _desc(m=N, n=N, ld=N, ctxt=0):
    return [1, ctxt, m, n, NB, NB, 0, 0, ld]


def _build_cases(daf):
    D = daf
    isz = {t: DT[t].itemsize for t in T4}
    rsz = {t: RT[t].itemsize for t in T4}
    sq = lambda K, name, t: K.arr(name, (N, N), DT[t])          # noqa: E731
    rh = lambda K, name, t: K.arr(name, (N, NRHS), DT[t])       # noqa: E731

    # -- the package root, grids, the distribution helpers
    case("initialize", lambda K: D.initialize())
    case("initialize[print_config]", lambda K: D.initialize(True))
    case("finalize", lambda K: D.finalize())
    case("version", lambda K: D.version())
    case("Grid.single", lambda K: D.Grid.single())
    case("Grid.rccl", lambda K: D.Grid.rccl(b"\x01\x02id", 4, 1, 2, 2, "C"))
    case("Grid.rccl_unique_id", lambda K: D.Grid.rccl_unique_id())
    case("Grid.host", lambda K: D.Grid.host(4, 1, 2, 2, "R", lambda axis, root, buf: None))
    case("Grid.barrier", lambda K: K.g1().barrier())
    case("Grid.selftest", lambda K: K.g1().selftest())
    case("Grid.selftest[64]", lambda K: K.g1().selftest(64))
    case("Grid.comm_log[on]", lambda K: K.g1().comm_log())
    case("Grid.comm_log[off]", lambda K: K.g1().comm_log(False))
    case("Grid.comm_log_events", lambda K: K.g1().comm_log_events())

    def free_twice(K):
        g = K.g1()
        g.free()
        g.free()
        return g.context
    case("Grid.free", free_twice)
    case("Grid.local_shape", lambda K: K.g4().local_shape(N, NB))
    case("Grid.local_shape[src]", lambda K: K.g4().local_shape(N, NB, 1, 1))
    ds = D.distribution
    case("distribution.rank_global_tile", lambda K: ds.rank_global_tile(5, 2, 1))
    case("distribution.local_tile_from_global_tile", lambda K: ds.local_tile_from_global_tile(5, 2, 1, 1))
    case("distribution.next_local_tile_from_global_tile", lambda K: ds.next_local_tile_from_global_tile(5, 2, 1))
    case("distribution.global_tile_from_local_tile", lambda K: ds.global_tile_from_local_tile(2, 2, 1, 1))
    case("distribution.local_size", lambda K: ds.local_size(N, NB, 2, 1))
    case("distribution.local_nr_tiles", lambda K: ds.local_nr_tiles(N, NB, 2, 1, 1))

    # -- the resident classes
    for t in T4:
        case(f"DeviceMatrix[{t}]", lambda K, t=t: D.DeviceMatrix(K.g1(), DT[t], "L", N, NB))
        case(f"GeneralDeviceMatrix[{t}]", lambda K, t=t: D.GeneralDeviceMatrix(K.g1(), DT[t], N, NRHS, NB))
    case("DeviceMatrix[z,U,src]", lambda K: D.DeviceMatrix(K.g4(), np.complex128, "U", N, NB, 1, 1))
    case("GeneralDeviceMatrix[z,src]", lambda K: D.GeneralDeviceMatrix(K.g4(), np.complex128, N, NRHS, NB, 1, 1))
    case("DeviceMatrix.upload", lambda K: K.dm("d").upload(sq(K, "a", "d")))
    case("DeviceMatrix.download", lambda K: K.dm("c").download(sq(K, "a", "c")))
    case("DeviceMatrix.fetch_tile", lambda K: K.dm("z").fetch_tile(1, 0), {3: NB * NB * 16})
    case("DeviceMatrix.copy_from", lambda K: K.dm("d").copy_from(K.dm("d")))
    case("DeviceMatrix.factorize", lambda K: K.dm("d").factorize())
    case("DeviceMatrix.generalized_to_standard", lambda K: K.dm("d").generalized_to_standard(K.dm("d")))
    case("DeviceMatrix.invert_triangular", lambda K: K.dm("d").invert_triangular())
    case("DeviceMatrix.invert_triangular[U,unit]", lambda K: K.dm("d", "U").invert_triangular("U"))
    case("DeviceMatrix.invert_from_factor", lambda K: K.dm("d").invert_from_factor())
    case("DeviceMatrix.to_general", lambda K: K.dm("d").to_general(K.gm("d", N, N)))
    case("DeviceMatrix.to_general[T]", lambda K: K.dm("d").to_general(K.gm("d", N, N), "T"))
    case("DeviceMatrix.from_general", lambda K: K.dm("d").from_general(K.gm("d", N, N)))
    case("DeviceMatrix.start", lambda K: K.dm("d").start())
    case("DeviceMatrix.wait", lambda K: K.dm("d").wait())
    case("DeviceMatrix.local_info", lambda K: K.dm("d").local_info())
    case("DeviceMatrix.residual_against", lambda K: K.dm("d").residual_against(K.dm("d")))
    for kind in ("update_bulk", "update_lookahead", "trsm_panel", "potrf_tile"):
        case(f"DeviceMatrix.profile[{kind}]", lambda K, kind=kind: K.dm("d").profile(kind))
    case("DeviceMatrix.trsm_profile", lambda K: K.dm("d").trsm_profile())
    case("DeviceMatrix.trsm_profile[3]", lambda K: K.dm("d").trsm_profile(3))

    def close_twice(K, make):
        m = make(K)
        m.close()
        m.close()
    case("DeviceMatrix.close", lambda K: close_twice(K, lambda K: K.dm("d")))
    case("GeneralDeviceMatrix.upload", lambda K: K.gm("s").upload(rh(K, "b", "s")))
    case("GeneralDeviceMatrix.download", lambda K: K.gm("z").download(rh(K, "b", "z")))
    case("GeneralDeviceMatrix.close", lambda K: close_twice(K, lambda K: K.gm("d")))

    # -- factorization
    for t in T4:
        case(f"cholesky_factorization[{t}]", lambda K, t=t: D.cholesky_factorization(K.g1(), "L", sq(K, "a", t), NB))
        case(f"pxpotrf[{t}]", lambda K, t=t: D.pxpotrf("L", N, sq(K, "a", t), 1, 1, _desc()))
        case(f"pxpotrs[{t}]", lambda K, t=t: D.pxpotrs("L", N, NRHS, sq(K, "a", t), 1, 1, _desc(), rh(K, "b", t), 1, 1,
                                                       _desc(N, NRHS)))
    case("cholesky_factorization[z,grid]",
         lambda K: D.cholesky_factorization(K.g4(), "Upper", sq(K, "a", "z")[:6, :4], NB, 1, 1, n=N))
    case("cholesky_factorization[no n]", lambda K: D.cholesky_factorization(K.g4(), "L", sq(K, "a", "d"), NB))
    case("cholesky_factorization[int32]", lambda K: D.cholesky_factorization(K.g1(), "L", K.arr("a", (N, N), np.int32), NB))
    case("cholesky_factorization[C order]",
         lambda K: D.cholesky_factorization(K.g1(), "L", np.ascontiguousarray(sq(K, "a", "d")), NB))
    case("pxpotrf[numpy descriptor]", lambda K: D.pxpotrf("U", N, sq(K, "a", "d"), 1, 1, list(np.array(_desc()))))
    case("set_random_hermitian_positive_definite",
         lambda K: D.set_random_hermitian_positive_definite(K.g1(), sq(K, "a", "c"), N, NB))
    case("set_random_hermitian_positive_definite[src,threads]",
         lambda K: D.set_random_hermitian_positive_definite(K.g4(), sq(K, "a", "d"), N, NB, 1, 1, 4))
    case("potrf_trace", lambda K: D.potrf_trace())
    case("update_launch_stats", lambda K: D.update_launch_stats())
    case("release_workspace_pool", lambda K: D.release_workspace_pool())
    case("potrs_device", lambda K: D.potrs_device("L", K.dm("d"), K.gm("d")))

    # -- triangular solver / multiplication
    for f in ("triangular_solver", "triangular_multiplication"):
        fn, fdev, px = getattr(D, f), getattr(D, f + "_device"), getattr(D, "pxtrsm" if f.endswith("solver") else "pxtrmm")
        for t in T4:
            case(f"{f}[{t}]", lambda K, t=t, fn=fn: fn(K.g1(), "L", "L", "N", "N", 2, sq(K, "a", t), rh(K, "b", t), NB),
                 {5: isz[t]})
            case(f"{px.__name__}[{t}]",
                 lambda K, t=t, px=px: px("L", "L", "N", "N", N, NRHS, 2, sq(K, "a", t), 1, 1, _desc(), rh(K, "b", t), 1, 1,
                                          _desc(N, NRHS)), {6: isz[t]})
            case(f"{f}_device[{t}]", lambda K, t=t, fdev=fdev: fdev("L", "L", "N", "N", 2, K.dm(t), K.gm(t)), {4: isz[t]})
        case(f"{f}[z,R]", lambda K, fn=fn: fn(K.g1(), "r", "U", "C", "U", 1 - 2j, K.arr("a", (NRHS, NRHS), DT["z"]),
                                              rh(K, "b", "z"), NB), {5: 16})
        case(f"{f}[z,grid]", lambda K, fn=fn: fn(K.g4(), "L", "L", "N", "N", 2, sq(K, "a", "z")[:4, :4], rh(K, "b", "z")[:4],
                                                 NB, N, NRHS, (1, 0), (0, 1), (NB, 2)), {5: 16})
        case(f"{f}[no sizes]", lambda K, fn=fn: fn(K.g4(), "L", "L", "N", "N", 2, sq(K, "a", "d"), rh(K, "b", "d"), NB))
        case(f"{f}[no n]", lambda K, fn=fn: fn(K.g4(), "L", "L", "N", "N", 2, sq(K, "a", "d"), rh(K, "b", "d"), NB, m=N))
        case(f"{f}[types differ]", lambda K, fn=fn: fn(K.g1(), "L", "L", "N", "N", 2, sq(K, "a", "s"), rh(K, "b", "d"), NB))

    # -- Hermitian and general multiplication
    for t in T4:
        case(f"hermitian_multiplication[{t}]",
             lambda K, t=t: D.hermitian_multiplication(K.g1(), "L", "L", 2, sq(K, "a", t), rh(K, "b", t), 3, rh(K, "c", t), NB),
             {3: isz[t], 8: isz[t]})
        case(f"pxhemm[{t}]",
             lambda K, t=t: D.pxhemm("L", "L", N, NRHS, 2, sq(K, "a", t), 1, 1, _desc(), rh(K, "b", t), 1, 1, _desc(N, NRHS), 3,
                                     rh(K, "c", t), 1, 1, _desc(N, NRHS)), {4: isz[t], 13: isz[t]})
        case(f"hermitian_multiplication_device[{t}]",
             lambda K, t=t: D.hermitian_multiplication_device("L", "L", 2, K.dm(t), K.gm(t), 3, K.gm(t)),
             {2: isz[t], 5: isz[t]})
        case(f"general_multiplication[{t}]",
             lambda K, t=t: D.general_multiplication(K.g1(), "N", "N", 2, K.arr("a", (N, 5), DT[t]),
                                                     K.arr("b", (5, NRHS), DT[t]), 3, rh(K, "c", t), NB),
             {3: isz[t], 8: isz[t]})
        case(f"pxgemm[{t}]",
             lambda K, t=t: D.pxgemm("N", "C", N, NRHS, 5, 2, K.arr("a", (N, 5), DT[t]), 1, 1, _desc(N, 5),
                                     K.arr("b", (NRHS, 5), DT[t]), 1, 1, _desc(NRHS, 5, NRHS), 3, rh(K, "c", t), 1, 1,
                                     _desc(N, NRHS)), {5: isz[t], 14: isz[t]})
        case(f"general_multiplication_device[{t}]",
             lambda K, t=t: D.general_multiplication_device("N", "T", 2, K.gm(t, N, 5), K.gm(t, NRHS, 5), 3, K.gm(t)),
             {2: isz[t], 5: isz[t]})
    case("hermitian_multiplication[z,R,grid]",
         lambda K: D.hermitian_multiplication(K.g4(), "R", "U", 2j, K.arr("a", (NRHS, NRHS), DT["z"]), rh(K, "b", "z")[:4],
                                              0.5, rh(K, "c", "z")[:6], NB, N, NRHS, (1, 0), (0, 1), (NB, 2)), {3: 16, 8: 16})
    case("hermitian_multiplication[z,R]",
         lambda K: D.hermitian_multiplication(K.g1(), "R", "U", 2j, K.arr("a", (NRHS, NRHS), DT["z"]), rh(K, "b", "z"), 0.5,
                                              rh(K, "c", "z"), NB), {3: 16, 8: 16})
    case("hermitian_multiplication[no sizes]",
         lambda K: D.hermitian_multiplication(K.g4(), "L", "L", 2, sq(K, "a", "d"), rh(K, "b", "d"), 3, rh(K, "c", "d"), NB))
    case("hermitian_multiplication[types differ]",
         lambda K: D.hermitian_multiplication(K.g1(), "L", "L", 2, sq(K, "a", "d"), rh(K, "b", "s"), 3, rh(K, "c", "d"), NB))
    for opa, opb in (("T", "N"), ("N", "C"), ("c", "t")):
        case(f"general_multiplication[z,{opa}{opb}]",
             lambda K, opa=opa, opb=opb: D.general_multiplication(
                 K.g1(), opa, opb, 2, K.arr("a", (N, 5) if opa == "N" else (5, N), DT["z"]),
                 K.arr("b", (5, NRHS) if opb == "N" else (NRHS, 5), DT["z"]), 3, rh(K, "c", "z"), NB), {3: 16, 8: 16})
    case("general_multiplication[d,grid]",
         lambda K: D.general_multiplication(K.g4(), "N", "N", 2, K.arr("a", (4, 5), DT["d"]), K.arr("b", (5, 2), DT["d"]), 3,
                                            rh(K, "c", "d")[:4, :2], NB, N, NRHS, 5, (1, 0), (0, 1), (1, 1)), {3: 8, 8: 8})
    case("general_multiplication[no sizes]",
         lambda K: D.general_multiplication(K.g4(), "N", "N", 2, K.arr("a", (N, 5), DT["d"]), K.arr("b", (5, NRHS), DT["d"]),
                                            3, rh(K, "c", "d"), NB, N, NRHS))
    case("general_multiplication[types differ]",
         lambda K: D.general_multiplication(K.g1(), "N", "N", 2, K.arr("a", (N, 5), DT["s"]), K.arr("b", (5, NRHS), DT["d"]),
                                            3, rh(K, "c", "d"), NB))
    case("multiplication_profile", lambda K: D.multiplication_profile())
    case("solver_profile", lambda K: D.solver_profile())

    # -- Hermitian rank-k / rank-2k updates
    for t in T4:
        case(f"hermitian_rank_k_update[{t}]",
             lambda K, t=t: D.hermitian_rank_k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT[t]), 3, sq(K, "c", t), NB),
             {3: rsz[t], 6: rsz[t]})
        case(f"hermitian_rank_2k_update[{t}]",
             lambda K, t=t: D.hermitian_rank_2k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT[t]),
                                                       K.arr("b", (N, 5), DT[t]), 3, sq(K, "c", t), NB),
             {3: isz[t], 8: rsz[t]})
        case(f"pxherk[{t}]",
             lambda K, t=t: D.pxherk("L", "N", N, 5, 2, K.arr("a", (N, 5), DT[t]), 1, 1, _desc(N, 5), 3, sq(K, "c", t), 1, 1,
                                     _desc()), {4: rsz[t], 9: rsz[t]})
        case(f"pxher2k[{t}]",
             lambda K, t=t: D.pxher2k("L", "N", N, 5, 2, K.arr("a", (N, 5), DT[t]), 1, 1, _desc(N, 5),
                                      K.arr("b", (N, 5), DT[t]), 1, 1, _desc(N, 5), 3, sq(K, "c", t), 1, 1, _desc()),
             {4: isz[t], 13: rsz[t]})
        case(f"hermitian_rank_k_update_device[{t}]",
             lambda K, t=t: D.hermitian_rank_k_update_device("L", "N", 2, K.gm(t, N, 5), 3, K.dm(t)), {2: rsz[t], 4: rsz[t]})
        case(f"hermitian_rank_2k_update_device[{t}]",
             lambda K, t=t: D.hermitian_rank_2k_update_device("L", "N", 2, K.gm(t, N, 5), K.gm(t, N, 5), 3, K.dm(t)),
             {2: isz[t], 5: rsz[t]})
    case("hermitian_rank_k_update[z,C]",
         lambda K: D.hermitian_rank_k_update(K.g1(), "U", "c", 2, K.arr("a", (5, N), DT["z"]), 3, sq(K, "c", "z"), NB),
         {3: 8, 6: 8})
    case("hermitian_rank_2k_update[z,C]",
         lambda K: D.hermitian_rank_2k_update(K.g1(), "U", "C", 2 + 1j, K.arr("a", (5, N), DT["z"]),
                                              K.arr("b", (5, N), DT["z"]), 3, sq(K, "c", "z"), NB), {3: 16, 8: 8})
    case("hermitian_rank_k_update[d,grid]",
         lambda K: D.hermitian_rank_k_update(K.g4(), "L", "N", 2, K.arr("a", (4, 3), DT["d"]), 3, sq(K, "c", "d")[:4, :4], NB,
                                             N, 5, (1, 0), (1, 1)), {3: 8, 6: 8})
    case("hermitian_rank_2k_update[d,grid]",
         lambda K: D.hermitian_rank_2k_update(K.g4(), "L", "N", 2, K.arr("a", (4, 3), DT["d"]), K.arr("b", (6, 3), DT["d"]), 3,
                                              sq(K, "c", "d")[:4, :4], NB, N, 5, (1, 0), (1, 1)), {3: 8, 8: 8})
    case("hermitian_rank_k_update[no sizes]",
         lambda K: D.hermitian_rank_k_update(K.g4(), "L", "N", 2, K.arr("a", (N, 5), DT["d"]), 3, sq(K, "c", "d"), NB, n=N))
    case("hermitian_rank_k_update[types differ]",
         lambda K: D.hermitian_rank_k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT["s"]), 3, sq(K, "c", "d"), NB))
    case("hermitian_rank_2k_update[types differ]",
         lambda K: D.hermitian_rank_2k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT["d"]), K.arr("b", (N, 5), DT["s"]), 3,
                                              sq(K, "c", "d"), NB))

    # -- addition, transposition, completion
    for t in T4:
        case(f"general_addition[{t}]",
             lambda K, t=t: D.general_addition(K.g1(), "A", "N", 2, rh(K, "a", t), 3, rh(K, "c", t), NB),
             {3: isz[t], 6: isz[t]})
        case(f"hermitian_complete[{t}]", lambda K, t=t: D.hermitian_complete(K.g1(), "L", "H", sq(K, "a", t), NB))
        case(f"pxgeadd[{t}]",
             lambda K, t=t: D.pxgeadd("N", N, NRHS, 2, rh(K, "a", t), 1, 1, _desc(N, NRHS), 3, rh(K, "c", t), 1, 1,
                                      _desc(N, NRHS)), {3: isz[t], 8: isz[t]})
        case(f"pxtradd[{t}]",
             lambda K, t=t: D.pxtradd("L", "N", N, NRHS, 2, rh(K, "a", t), 1, 1, _desc(N, NRHS), 3, rh(K, "c", t), 1, 1,
                                      _desc(N, NRHS)), {4: isz[t], 9: isz[t]})
        for conj in (False, True):
            case(f"pxtran[{t},conj={conj}]",
                 lambda K, t=t, conj=conj: D.pxtran(N, NRHS, 2, K.arr("a", (NRHS, N), DT[t]), 1, 1, _desc(NRHS, N, NRHS), 3,
                                                    rh(K, "c", t), 1, 1, _desc(N, NRHS), conj), {2: isz[t], 7: isz[t]})
        case(f"pxlacpy[{t}]",
             lambda K, t=t: D.pxlacpy("U", N, NRHS, rh(K, "a", t), 1, 1, _desc(N, NRHS), rh(K, "b", t), 1, 1, _desc(N, NRHS)))
        case(f"general_addition_device[{t}]",
             lambda K, t=t: D.general_addition_device("A", "N", 2, K.gm(t), 3, K.gm(t)), {2: isz[t], 4: isz[t]})
    case("general_addition[z,C,grid]",
         lambda K: D.general_addition(K.g4(), "U", "C", 2j, K.arr("a", (2, 4), DT["z"]), 3, rh(K, "c", "z")[:4, :2], NB, N, NRHS,
                                      (1, 0), (0, 1)), {3: 16, 6: 16})
    case("general_addition[z,T]",
         lambda K: D.general_addition(K.g1(), "L", "t", 2j, K.arr("a", (NRHS, N), DT["z"]), 3, rh(K, "c", "z"), NB),
         {3: 16, 6: 16})
    case("general_addition[no sizes]",
         lambda K: D.general_addition(K.g4(), "A", "N", 2, rh(K, "a", "d"), 3, rh(K, "c", "d"), NB))
    case("general_addition[types differ]",
         lambda K: D.general_addition(K.g1(), "A", "N", 2, rh(K, "a", "s"), 3, rh(K, "c", "d"), NB))
    case("hermitian_complete[z,U,S,grid]",
         lambda K: D.hermitian_complete(K.g4(), "U", "S", sq(K, "a", "z")[:4, :4], NB, N, (1, 1)))
    case("hermitian_complete[no n]", lambda K: D.hermitian_complete(K.g4(), "L", "H", sq(K, "a", "d"), NB))
    case("hermitian_complete_device", lambda K: D.hermitian_complete_device("U", "S", K.gm("c", N, N)))
    case("addition_profile", lambda K: D.addition_profile())

    # -- gen_to_std and the inverses
    for t in T4:
        case(f"generalized_to_standard[{t}]",
             lambda K, t=t: D.generalized_to_standard(K.g1(), "L", sq(K, "a", t), sq(K, "b", t), NB))
        case(f"pxhegst[{t}]",
             lambda K, t=t: D.pxhegst(1, "L", N, sq(K, "a", t), 1, 1, _desc(), sq(K, "b", t), 1, 1, _desc()))
        case(f"triangular_inverse[{t}]", lambda K, t=t: D.triangular_inverse(K.g1(), "L", "N", sq(K, "a", t), NB))
        case(f"inverse_from_cholesky_factor[{t}]",
             lambda K, t=t: D.inverse_from_cholesky_factor(K.g1(), "L", sq(K, "a", t), NB))
        case(f"pxtrtri[{t}]", lambda K, t=t: D.pxtrtri("U", "U", N, sq(K, "a", t), 1, 1, _desc()))
        case(f"pxpotri[{t}]", lambda K, t=t: D.pxpotri("U", N, sq(K, "a", t), 1, 1, _desc()))
    case("generalized_to_standard[z,grid]",
         lambda K: D.generalized_to_standard(K.g4(), "U", sq(K, "a", "z")[:4, :4], sq(K, "b", "z")[:6, :4], NB, 1, 1, N))
    case("generalized_to_standard[no n]",
         lambda K: D.generalized_to_standard(K.g4(), "L", sq(K, "a", "d"), sq(K, "b", "d"), NB))
    case("generalized_to_standard[types differ]",
         lambda K: D.generalized_to_standard(K.g1(), "L", sq(K, "a", "d"), sq(K, "b", "s"), NB))
    case("triangular_inverse[z,grid]",
         lambda K: D.triangular_inverse(K.g4(), "U", "U", sq(K, "a", "z")[:4, :4], NB, 1, 1, N))
    case("triangular_inverse[no n]", lambda K: D.triangular_inverse(K.g4(), "L", "N", sq(K, "a", "d"), NB))
    case("inverse_from_cholesky_factor[z,grid]",
         lambda K: D.inverse_from_cholesky_factor(K.g4(), "U", sq(K, "a", "z")[:4, :4], NB, 1, 1, N))
    case("inverse_from_cholesky_factor[no n]", lambda K: D.inverse_from_cholesky_factor(K.g4(), "L", sq(K, "a", "d"), NB))
    case("inverse_profile", lambda K: D.inverse_profile())

    # -- norms
    for t in T4:
        for s in "GHT":
            case(f"matrix_norm[{t},{s}]",
                 lambda K, t=t, s=s: D.matrix_norm(K.g1(), "F", rh(K, "a", t) if s == "G" else sq(K, "a", t), NB, s))
        case(f"pxlange[{t}]", lambda K, t=t: D.pxlange("M", N, NRHS, rh(K, "a", t), 1, 1, _desc(N, NRHS)))
        case(f"pxlanhe[{t}]", lambda K, t=t: D.pxlanhe("1", "U", N, sq(K, "a", t), 1, 1, _desc()))
        case(f"pxlantr[{t}]", lambda K, t=t: D.pxlantr("I", "L", "U", N, sq(K, "a", t), 1, 1, _desc()))
    case("matrix_norm[d,s,grid]",
         lambda K: D.matrix_norm(K.g4(), "1", sq(K, "a", "d")[:4, :4], NB, "s", "U", "N", N, N, 1, 1))
    case("matrix_norm[d,T,unit]", lambda K: D.matrix_norm(K.g1(), "I", sq(K, "a", "d"), NB, "T", "U", "U"))
    case("matrix_norm[no sizes]", lambda K: D.matrix_norm(K.g4(), "M", sq(K, "a", "d"), NB))
    case("matrix_norm[bad structure]", lambda K: D.matrix_norm(K.g1(), "M", sq(K, "a", "d"), NB, "X"))
    case("matrix_norm_device[general]", lambda K: D.matrix_norm_device("F", K.gm("d")))
    case("matrix_norm_device[general,H]", lambda K: D.matrix_norm_device("F", K.gm("d"), "H"))
    case("matrix_norm_device[hermitian]", lambda K: D.matrix_norm_device("1", K.dm("z")))
    case("matrix_norm_device[triangular]", lambda K: D.matrix_norm_device("I", K.dm("z"), "T", "U"))
    case("norm_profile", lambda K: D.norm_profile())

    # -- the tile operations and the direct doors of the kernels
    for t in T4:
        case(f"tile_potrf[{t}]", lambda K, t=t: D.tile_potrf("L", K.arr("a", (NB, NB), DT[t])))
        case(f"update_bulk_slots[{t}]", lambda K, t=t: D.update_bulk_slots(DT[t]))
        case(f"update_direct[{t}]",
             lambda K, t=t: D.update_direct(K.arr("c", 16, DT[t]), K.arr("a", 16, DT[t]), K.arr("b", 16, DT[t]), nb=NB, K=NB,
                                            ldc=NB, lda=NB, ldb=NB, il1=1, jl1=1))
        case(f"trsm_direct[{t}]",
             lambda K, t=t: D.trsm_direct(K.arr("b", 32, DT[t]), K.arr("l", 16, DT[t]), K.arr("w", 16, DT[t]), nb=NB, ldb=N,
                                          ldl=NB, n=NB, il1=2))
        case(f"potrf_direct[{t}]",
             lambda K, t=t: D.potrf_direct(K.arr("t", 16, DT[t]), K.arr("w", 16, DT[t]), kb=NB, ld=NB))
    for u in "LU":
        case(f"tile_trsm[d,{u}]", lambda K, u=u: D.tile_trsm(u, K.arr("a", (NB, NB), DT["d"]), K.arr("b", (3, NB), DT["d"])))
        case(f"tile_herk[z,{u}]", lambda K, u=u: D.tile_herk(u, K.arr("a", (NB, 3) if u == "L" else (3, NB), DT["z"]),
                                                             K.arr("c", (NB, NB), DT["z"])))
        case(f"tile_gemm[c,{u}]",
             lambda K, u=u: D.tile_gemm(u, K.arr("a", (NB, 3) if u == "L" else (3, NB), DT["c"]),
                                        K.arr("b", (2, 3) if u == "L" else (3, 2), DT["c"]), K.arr("c", (NB, 2), DT["c"])))
    case("update_direct[d,K1,repeat]",  # (c_again is uninitialised memory behind the stand-in: its shape only)
         lambda K: (lambda r: (r[0], r[1], r[2].shape))(D.update_direct(
             K.arr("c", 16, DT["d"]), K.arr("a", 16, DT["d"]), K.arr("b", 16, DT["d"]), a2=K.arr("a2", 8, DT["d"]),
             b2=K.arr("b2", 8, DT["d"]), offsets=(1, 2, 3, 4, 5), repeat=True, nb=NB, K=NB, K1=2, her2k=1, max_blocks=3,
             b_period=2)), {6: OPAQUE})
    case("update_direct[unknown field]",
         lambda K: D.update_direct(K.arr("c", 16, DT["d"]), K.arr("a", 16, DT["d"]), K.arr("b", 16, DT["d"]), kb=4))
    case("update_direct[not flat]",
         lambda K: D.update_direct(K.arr("c", (4, 4), DT["d"]), K.arr("a", 16, DT["d"]), K.arr("b", 16, DT["d"])))
    case("trsm_direct[z,caller,offsets]",
         lambda K: D.trsm_direct(K.arr("b", 32, DT["z"]), K.arr("l", 16, DT["z"]), K.arr("w", 16, DT["z"]),
                                 winv_source="caller", offsets=(1, 2, 3), nb=NB, upper=1, unit=1))
    case("trsm_direct[unknown field]",
         lambda K: D.trsm_direct(K.arr("b", 32, DT["d"]), K.arr("l", 16, DT["d"]), K.arr("w", 16, DT["d"]), kb=4))
    case("trsm_direct[types differ]",
         lambda K: D.trsm_direct(K.arr("b", 32, DT["d"]), K.arr("l", 16, DT["s"]), K.arr("w", 16, DT["d"])))
    case("potrf_direct[z,chain,offsets]",
         lambda K: D.potrf_direct(K.arr("t", 16, DT["z"]), K.arr("w", 16, DT["z"]), path="chain", offsets=(3, 5), kb=NB, ld=NB,
                                  info_base=7, count_strips=1))
    case("potrf_direct[unknown field]",
         lambda K: D.potrf_direct(K.arr("t", 16, DT["d"]), K.arr("w", 16, DT["d"]), nb=4))
    case("potrf_direct[not flat]", lambda K: D.potrf_direct(K.arr("t", (4, 4), DT["d"]), K.arr("w", 16, DT["d"])))

    # -- the eigensolver stages
    case("get_band_size", lambda K: D.get_band_size(NB))
    case("red2band_panel_stats", lambda K: D.red2band_panel_stats())
    case("eigensolver_min_band", lambda K: D.eigensolver_min_band())
    case("eigensolver_min_band[set]", lambda K: D.eigensolver_min_band(32))
    case("red2band_profile", lambda K: D.red2band_profile())
    case("eigensolver_profile", lambda K: D.eigensolver_profile())
    case("sturm_layout", lambda K: D.sturm_layout())
    case("partial_spectrum_plan", lambda K: D.partial_spectrum_plan(N, NB, 2, 1, 0, 2, 6))
    for t in T4:
        case(f"reduction_to_band[{t}]", lambda K, t=t: D.reduction_to_band(K.g1(), sq(K, "a", t), NB, 2), {4: 5 * isz[t]})
        case(f"bt_reduction_to_band[{t}]",
             lambda K, t=t: D.bt_reduction_to_band(K.g1(), 2, rh(K, "c", t), sq(K, "v", t), K.arr("taus", 5, DT[t]), NB))
        case(f"band_to_tridiagonal[{t}]", lambda K, t=t: D.band_to_tridiagonal(K.g1(), sq(K, "a", t), NB, 2),
             {4: N * rsz[t], 5: N * rsz[t], 6: N * N * isz[t]})
        case(f"bt_band_to_tridiagonal[{t}]", lambda K, t=t: D.bt_band_to_tridiagonal(2, rh(K, "e", t), sq(K, "v", t)))
        case(f"reduction_to_band_device[{t}]", lambda K, t=t: D.reduction_to_band_device(K.dm(t), 2), {2: 5 * isz[t]})
        case(f"bt_reduction_to_band_device[{t}]",
             lambda K, t=t: D.bt_reduction_to_band_device(2, K.gm(t), K.dm(t), K.arr("taus", 5, DT[t])))
    case("reduction_to_band[z,grid]",
         lambda K: D.reduction_to_band(K.g4(), sq(K, "a", "z")[:4, :4], NB, 2, 1, 1, N), {4: 5 * 16})
    case("reduction_to_band[no n]", lambda K: D.reduction_to_band(K.g4(), sq(K, "a", "d"), NB, 2))
    case("bt_reduction_to_band[z,grid]",
         lambda K: D.bt_reduction_to_band(K.g4(), 2, rh(K, "c", "z")[:4, :2], sq(K, "v", "z")[:6, :4], K.arr("taus", 5, DT["z"]),
                                          NB, 1, 0, 1, N, NRHS))
    case("bt_reduction_to_band[no sizes]",
         lambda K: D.bt_reduction_to_band(K.g4(), 2, rh(K, "c", "d"), sq(K, "v", "d"), K.arr("taus", 5, DT["d"]), NB, n=N))
    case("band_to_tridiagonal[z,grid]", lambda K: D.band_to_tridiagonal(K.g4(), sq(K, "a", "z")[:4, :4], NB, 2, 1, 1, N),
         {4: N * 8, 5: N * 8, 6: N * N * 16})
    case("band_to_tridiagonal[no n]", lambda K: D.band_to_tridiagonal(K.g4(), sq(K, "a", "d"), NB, 2))
    for t in "sd":
        case(f"tridiagonal_eigensolver[{t}]",
             lambda K, t=t: D.tridiagonal_eigensolver(K.arr("d", N, DT[t]), K.arr("e", N - 1, DT[t]), NB),
             {4: N * isz[t], 5: N * N * isz[t]})
        case(f"tridiagonal_eigensolver[{t},index]",
             lambda K, t=t: D.tridiagonal_eigensolver(K.arr("d", N, DT[t]), K.arr("e", N - 1, DT[t]), NB, (2, 5)),
             {4: N * isz[t], 5: N * 3 * isz[t]})
        case(f"tridiagonal_eigenvalues[{t}]",
             lambda K, t=t: D.tridiagonal_eigenvalues(K.arr("d", N, DT[t]), K.arr("e", N - 1, DT[t])), {3: N * isz[t]})
        case(f"tridiagonal_sturm_count[{t}]",
             lambda K, t=t: D.tridiagonal_sturm_count(K.arr("d", N, DT[t]), K.arr("e", N - 1, DT[t]), K.arr("shifts", 3, DT[t])),
             {5: 3 * 8})
    case("tridiagonal_eigensolver[d,index,z]",
         lambda K: D.tridiagonal_eigensolver(K.arr("d", N, DT["d"]), K.arr("e", N - 1, DT["d"]), NB, (2, 5), sq(K, "z", "d")),
         {4: N * 8})
    case("tridiagonal_eigenvalues[d,index,w]",
         lambda K: D.tridiagonal_eigenvalues(K.arr("d", N, DT["d"]), K.arr("e", N - 1, DT["d"]), (np.int64(2), 5),
                                             K.arr("w", N, DT["d"])))
    case("tridiagonal_sturm_count[d,list]",
         lambda K: D.tridiagonal_sturm_count(K.arr("d", N, DT["d"]), K.arr("e", N - 1, DT["d"]), [0.5, 1.5]),
         {4: 2 * 8, 5: 2 * 8})

    # -- the eigensolver drivers
    for t in T4:
        case(f"hermitian_eigenvalues[{t}]", lambda K, t=t: D.hermitian_eigenvalues(K.g1(), "L", sq(K, "a", t), NB),
             {4: N * rsz[t]})
        case(f"hermitian_eigensolver[{t}]", lambda K, t=t: D.hermitian_eigensolver(K.g1(), "L", sq(K, "a", t), NB),
             {4: N * rsz[t], 5: N * N * isz[t]})
        case(f"hermitian_eigensolver[{t},index]",
             lambda K, t=t: D.hermitian_eigensolver(K.g1(), "L", sq(K, "a", t), NB, eigenvalues_index=(2, 5)),
             {4: N * rsz[t], 5: N * N * isz[t]})
        case(f"hermitian_eigensolver[{t},value]",
             lambda K, t=t: D.hermitian_eigensolver(K.g1(), "L", sq(K, "a", t), NB, eigenvalues_value=(-1, 2.5)),
             {4: N * rsz[t], 5: N * N * isz[t]})
        for fac in (False, True):
            case(f"hermitian_generalized_eigenvalues[{t},factorized={fac}]",
                 lambda K, t=t, fac=fac: D.hermitian_generalized_eigenvalues(K.g1(), "L", sq(K, "a", t), sq(K, "b", t), NB,
                                                                             factorized=fac), {6: N * rsz[t]})
            case(f"hermitian_generalized_eigensolver[{t},factorized={fac}]",
                 lambda K, t=t, fac=fac: D.hermitian_generalized_eigensolver(K.g1(), "L", sq(K, "a", t), sq(K, "b", t), NB,
                                                                             factorized=fac),
                 {6: N * rsz[t], 7: N * N * isz[t]})
            for sel in ("index", "value") if t == "z" or not fac else ():  # (factorized x selection: on one type)
                case(f"hermitian_generalized_eigensolver[{t},factorized={fac},{sel}]",
                     lambda K, t=t, fac=fac, sel=sel: D.hermitian_generalized_eigensolver(
                         K.g1(), "L", sq(K, "a", t), sq(K, "b", t), NB, factorized=fac,
                         **({"eigenvalues_index": (2, 5)} if sel == "index" else {"eigenvalues_value": (-1, 2.5)})),
                     {6: N * rsz[t], 7: N * N * isz[t]})
            case(f"pxhegvd_eigenvalues[{t},factorized={fac}]",
                 lambda K, t=t, fac=fac: D.pxhegvd_eigenvalues("L", sq(K, "a", t), _desc(), sq(K, "b", t), _desc(), 2, 5, N, fac),
                 {10: N * rsz[t]})
            case(f"pxhegvd_partial_spectrum_by_value[{t},factorized={fac}]",
                 lambda K, t=t, fac=fac: D.pxhegvd_partial_spectrum_by_value(
                     "L", sq(K, "a", t), _desc(), sq(K, "b", t), _desc(), sq(K, "z", t), _desc(), -1, 2.5, N, fac),
                 {10: N * rsz[t]})
        case(f"pxheevd_partial_spectrum[{t}]",
             lambda K, t=t: D.pxheevd_partial_spectrum("L", sq(K, "a", t), _desc(), sq(K, "z", t), _desc(), 2, 5, N),
             {6: N * rsz[t]})
        case(f"pxheevd_eigenvalues[{t}]", lambda K, t=t: D.pxheevd_eigenvalues("L", sq(K, "a", t), _desc(), 2, 5, N),
             {6: N * rsz[t]})
        case(f"pxheevd_partial_spectrum_by_value[{t}]",
             lambda K, t=t: D.pxheevd_partial_spectrum_by_value("L", sq(K, "a", t), _desc(), sq(K, "z", t), _desc(), -1, 2.5, N),
             {6: N * rsz[t]})
    case("hermitian_eigenvalues[z,grid,index,w]",
         lambda K: D.hermitian_eigenvalues(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], NB, 1, 1, N, (2, 5), K.arr("w", N, DT["d"])))
    case("hermitian_eigenvalues[no n]", lambda K: D.hermitian_eigenvalues(K.g4(), "L", sq(K, "a", "d"), NB))
    case("hermitian_generalized_eigenvalues[z,grid,index,w]",
         lambda K: D.hermitian_generalized_eigenvalues(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], sq(K, "b", "z")[:6, :4], NB, 1, 1,
                                                       N, False, (2, 5), K.arr("w", N, DT["d"])))
    case("hermitian_generalized_eigenvalues[no n]",
         lambda K: D.hermitian_generalized_eigenvalues(K.g4(), "L", sq(K, "a", "d"), sq(K, "b", "d"), NB))
    case("hermitian_eigensolver[z,grid,z]",
         lambda K: D.hermitian_eigensolver(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], NB, 1, 1, N, 0, None, None,
                                           sq(K, "z", "z")[:6, :4]), {4: N * 8})
    case("hermitian_eigensolver[d,z_shape]",
         lambda K: D.hermitian_eigensolver(K.g4(), "L", sq(K, "a", "d")[:4, :4], NB, n=N, z_jsrc=1, z_shape=(4, 2)),
         {4: N * 8, 5: 4 * 2 * 8})
    case("hermitian_eigensolver[no n]", lambda K: D.hermitian_eigensolver(K.g4(), "L", sq(K, "a", "d"), NB))
    case("hermitian_eigensolver[both selections]",
         lambda K: D.hermitian_eigensolver(K.g1(), "L", sq(K, "a", "d"), NB, eigenvalues_index=(0, 1), eigenvalues_value=(0, 1)))
    case("hermitian_generalized_eigensolver[z,grid,z]",
         lambda K: D.hermitian_generalized_eigensolver(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], sq(K, "b", "z")[:6, :4], NB, 1,
                                                       1, N, False, None, sq(K, "z", "z")[:5, :4]), {6: N * 8})
    case("hermitian_generalized_eigensolver[no n]",
         lambda K: D.hermitian_generalized_eigensolver(K.g4(), "L", sq(K, "a", "d"), sq(K, "b", "d"), NB))
    case("hermitian_generalized_eigensolver[both selections]",
         lambda K: D.hermitian_generalized_eigensolver(K.g1(), "L", sq(K, "a", "d"), sq(K, "b", "d"), NB,
                                                       eigenvalues_index=(0, 1), eigenvalues_value=(0, 1)))
    case("pxheevd_eigenvalues[d,w]",
         lambda K: D.pxheevd_eigenvalues("Lower", sq(K, "a", "d"), _desc(), 2, 5, N, K.arr("w", N, DT["d"])))
    case("pxhegvd_eigenvalues[d,w]",
         lambda K: D.pxhegvd_eigenvalues("Lower", sq(K, "a", "d"), _desc(), sq(K, "b", "d"), _desc(), 2, 5, N,
                                         w=K.arr("w", N, DT["d"])))

    # -- the weighted rank-k update and the matrix functions
    fn = lambda lam: lam  # noqa: E731
    for t in T4:
        case(f"hermitian_weighted_rank_k_update[{t}]",
             lambda K, t=t: D.hermitian_weighted_rank_k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT[t]),
                                                               K.arr("d", 5, RT[t]), 3, sq(K, "c", t), NB),
             {3: rsz[t], 7: rsz[t]})
        case(f"hermitian_weighted_rank_k_update_device[{t}]",
             lambda K, t=t: D.hermitian_weighted_rank_k_update_device("L", "N", 2, K.gm(t, N, 5), K.arr("d", 5, RT[t]), 3,
                                                                      K.dm(t)), {2: rsz[t], 5: rsz[t]})
        case(f"hermitian_function[{t}]", lambda K, t=t: D.hermitian_function(K.g1(), "L", sq(K, "a", t), NB, fn),
             {4: N * rsz[t], 9: 16})
        case(f"hermitian_function_device[{t}]", lambda K, t=t: D.hermitian_function_device(K.dm(t), fn),
             {1: N * rsz[t], 2: OPAQUE, 6: 16})
        case(f"hermitian_power[{t}]", lambda K, t=t: D.hermitian_power(K.g1(), "L", sq(K, "a", t), NB, -0.5),
             {4: N * rsz[t]})
        case(f"hermitian_power_device[{t}]", lambda K, t=t: D.hermitian_power_device(K.dm(t), -1, 1e-3), {1: N * rsz[t]})
    case("hermitian_weighted_rank_k_update[z,C,list]",
         lambda K: D.hermitian_weighted_rank_k_update(K.g1(), "U", "C", 2, K.arr("a", (5, N), DT["z"]), [1, -2, 3, 4, 5], 3,
                                                      sq(K, "c", "z"), NB), {3: 8, 6: 5 * 8, 7: 8})
    case("hermitian_weighted_rank_k_update[d,grid,no d]",
         lambda K: D.hermitian_weighted_rank_k_update(K.g4(), "L", "N", 2, K.arr("a", (4, 3), DT["d"]), None, 3,
                                                      sq(K, "c", "d")[:4, :4], NB, N, 5, (1, 0), (1, 1)), {3: 8, 7: 8})
    case("hermitian_weighted_rank_k_update[no sizes]",
         lambda K: D.hermitian_weighted_rank_k_update(K.g4(), "L", "N", 2, K.arr("a", (N, 5), DT["d"]), None, 3,
                                                      sq(K, "c", "d"), NB))
    case("hermitian_weighted_rank_k_update[types differ]",
         lambda K: D.hermitian_weighted_rank_k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT["s"]), None, 3,
                                                      sq(K, "c", "d"), NB))
    case("hermitian_weighted_rank_k_update[weights count]",
         lambda K: D.hermitian_weighted_rank_k_update(K.g1(), "L", "N", 2, K.arr("a", (N, 5), DT["d"]), [1, 2], 3,
                                                      sq(K, "c", "d"), NB))
    case("hermitian_weighted_rank_k_update_device[z,C]",
         lambda K: D.hermitian_weighted_rank_k_update_device("U", "C", 2, K.gm("z", 5, N), K.arr("d", 5, RT["z"]), 3,
                                                             K.dm("z", "U")), {2: 8, 5: 8})
    case("hermitian_function[z,grid,index]",
         lambda K: D.hermitian_function(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], NB, fn, 1, 1, N, eigenvalues_index=(2, 5)),
         {4: N * 8, 7: 16, 9: 16})
    case("hermitian_function[c,value]",
         lambda K: D.hermitian_function(K.g1(), "L", sq(K, "a", "c"), NB, fn, eigenvalues_value=(-1, 2.5)),
         {4: N * 4, 8: 8, 9: 16})
    case("hermitian_function[no n]", lambda K: D.hermitian_function(K.g4(), "L", sq(K, "a", "d"), NB, fn))
    case("hermitian_function[both selections]",
         lambda K: D.hermitian_function(K.g1(), "L", sq(K, "a", "d"), NB, fn, eigenvalues_index=(0, 1), eigenvalues_value=(0, 1)))
    case("hermitian_function_device[d,index]", lambda K: D.hermitian_function_device(K.dm("d"), fn, eigenvalues_index=(2, 5)),
         {1: N * 8, 2: OPAQUE, 4: 16, 6: 16})
    case("hermitian_function_device[s,value]", lambda K: D.hermitian_function_device(K.dm("s"), fn, eigenvalues_value=(-1, 2.5)),
         {1: N * 4, 2: OPAQUE, 5: 8, 6: 16})
    case("hermitian_power[z,grid]",
         lambda K: D.hermitian_power(K.g4(), "Lower", sq(K, "a", "z")[:4, :4], NB, -1, 1e-3, 1, 1, N), {4: N * 8})
    case("hermitian_power[no n]", lambda K: D.hermitian_power(K.g4(), "L", sq(K, "a", "d"), NB, -1))


def _run_case(rec, daf, fn, scal, ret):
    K = Fixtures(rec, daf)
    rec._log, rec._arrays, rec._scal, rec._handles, rec._ret = [], K.arrays, scal, [], ret
    made = None
    try:
        made = fn(K)
        out = "= " + _result(made)
    except HarnessError:
        raise
    except Exception as e:
        out = f"! {type(e).__name__}: {e}".replace(PREFIX, "~")
    calls, rec._log = rec._log, None
    if hasattr(made, "close"):  # a resident matrix the case itself made: released with the log off, not by the collector
        K._keep.append(made)
    K.close()
    return calls, out


def record():
    """{"calls": {case id: {...}}, "signatures": {symbol: text}} of the dla_future_amd this interpreter imports."""
    import dla_future_amd as daf
    from dla_future_amd import capi
    saved = capi._lib
    rec = Recorder(capi)
    capi._lib = rec
    try:
        if not CASES:
            _build_cases(daf)
        calls = {}
        for cid, fn, scal in CASES:
            if cid in calls:
                raise HarnessError(f"duplicate case {cid}")
            try:
                first, out0 = _run_case(rec, daf, fn, scal, 0)
                again, out7 = _run_case(rec, daf, fn, scal, 7)
            except HarnessError as e:
                raise HarnessError(f"{cid}: {e}") from None
            # [the calls, the outcome when all succeed, the outcome when c_int entries return 7 (+ how many calls were
            #  made then, where that differs)]
            for k, c in enumerate(first):  # an outcome names a call of its case as $k
                out0, out7 = (o.replace(c.split("(")[0], f"${k}") for o in (out0, out7))
            calls[cid] = [first, out0, out7] + ([len(again)] if len(again) != len(first) else [])
    finally:
        capi._lib = saved
    return {"calls": calls, "signatures": signatures(capi), "structures": structures(capi)}


def dumps(log) -> str:
    """One line per entry, keys sorted: identical bytes for identical logs."""
    parts = []
    for section in sorted(log):
        lines = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(log[section].items()))
        parts.append(f"{json.dumps(section)}: {{\n{lines}\n}}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    text = dumps(record())
    with open(sys.argv[1], "w") as f:
        f.write(text)
    covered = {c.split("(")[0].replace("~", PREFIX) for e in json.loads(text)["calls"].values() for c in e[0]}
    print(f"{len(CASES)} cases, {len(covered)} entry points reached, {len(text)} bytes")
