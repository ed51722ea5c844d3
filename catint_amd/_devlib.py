"""What the ctypes bindings of the satellite libraries (every ``_*.py`` of this package beside ``_capi.py``) share: the mirror of
``pnp_device_view``, the pointer types and array helpers, a library's error class and its cached loader with the five lifecycle symbols
and the entry point, the handle class, and the two steps every ``solve`` takes around its call: the check of the requested field names
and the allocation of the result arrays."""
import ctypes as C
import os

import numpy as np

EINVAL, ENOMEM, EDEVICE = -1, -2, -3
_PD, _PI, _PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class PnpDeviceView(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('method', C.c_int32), ('nspecies', C.c_int32), ('nx', C.c_int32), ('row_pitch', C.c_int32),
                ('reserved', C.c_int32), ('batch', C.c_int64), ('c_dev', C.c_void_p), ('phi_dev', C.c_void_p), ('status_dev', C.c_void_p),
                ('stream', C.c_void_p)]


def _dptr(a):
    return a.ctypes.data_as(_PD) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _lptr(a):
    return a.ctypes.data_as(_PL) if a is not None else None


_cptr = _dptr          # a complex128 array as the (re, im) pairs of doubles the libraries write


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def lane_list(lanes):
    """lanes as the contiguous int64 list the libraries take, None as it is"""
    return None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)


def size_of(struct, given):
    """struct_size of a call: that of the mirror unless a test gives another"""
    return C.sizeof(struct) if given is None else int(given)


def field_names(fields, known, default=None):
    """the requested names as a list (None: `default`, or all of `known`), every one checked against `known`"""
    names = list(known if default is None else default) if fields is None else list(fields)
    for name in names:
        if name not in known:
            raise ValueError('unknown field %r (known: %s)' % (name, ', '.join(known)))
    return names


def results(out, shapes, lead, dtype=np.float64, status=None):
    """the dict a solve returns: `out` or a new one, with an array [lead..][shapes[name]..] of `dtype` for every name of `shapes` that
    has none and, with status = its shape, the int32 'status' row"""
    res = {} if out is None else out
    for name, shape in shapes.items():
        res.setdefault(name, np.empty(tuple(lead) + tuple(shape), dtype))
    if status is not None:
        res.setdefault('status', np.zeros(status, np.int32))
    return res


def lib_path(name):
    """Where libcatint_<name>.so is looked for: CATINT_<NAME>_LIB (diagnosis builds of tools/probe) or this package's lib/"""
    return os.environ.get('CATINT_%s_LIB' % name.upper()) or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib',
                                                                           'libcatint_%s.so' % name)


def symbols(prefix, entry):
    """Every symbol the library's header declares"""
    return [prefix + n for n in ('create', 'destroy', 'last_error', 'last_kernel', 'last_kernel_ms', entry)]


class LibraryError(RuntimeError):
    """A library's error: a binding module derives its own and names the library ('catint_response')"""
    library = None

    def __init__(self, code, msg):
        super().__init__('%s error %d: %s' % (self.library, code, msg))
        self.code = code


def load(path, prefix, entry, params, outputs, error):
    """CDLL of `path` with the argument and result types of <prefix>create .. <prefix>last_kernel_ms and of
    <prefix><entry>(ctx, view, params, outputs).  No fallback: a missing library raises `error`."""
    if not os.path.exists(path):
        raise error(EDEVICE, 'HIP extension %s is missing: run `python -c "import __graft_entry__ as g; g.build()"`' % path)
    lib = C.CDLL(path)
    for name, argtypes, restype in (('create', [C.c_int32, C.POINTER(C.c_void_p)], C.c_int), ('destroy', [C.c_void_p], None),
                                    ('last_error', [C.c_void_p], C.c_char_p), ('last_kernel', [C.c_void_p], C.c_char_p),
                                    ('last_kernel_ms', [C.c_void_p], C.c_float),
                                    (entry, [C.c_void_p, C.POINTER(PnpDeviceView), C.POINTER(params), C.POINTER(outputs)], C.c_int)):
        f = getattr(lib, prefix + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


def loader(ns, prefix, entry, params, outputs, error, more=()):
    """The load_library of a binding module, ns = its globals(): `load` of the module's LIB_PATH (as it stands at the first call) once,
    kept in the module's `_lib`.  more: further entry points with the signature of `entry` (cateis_solve)."""
    ns.setdefault('_lib', None)

    def load_library():
        if ns['_lib'] is None:
            lib = load(ns['LIB_PATH'], prefix, entry, params, outputs, error)
            for name in more:
                f = getattr(lib, prefix + name)
                f.argtypes, f.restype = getattr(lib, prefix + entry).argtypes, C.c_int
            ns['_lib'] = lib
        return ns['_lib']
    return load_library


class Handle(object):
    """One context of a library.  A subclass names its symbols' prefix, its error class and its load_library."""
    _prefix = None
    _error = None
    _load = None

    def __init__(self, device=0):
        self._lib = type(self)._load()
        self._h = C.c_void_p()
        rc = self._sym('create')(int(device), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise self._error(rc, self._sym('last_error')(None).decode())

    def _sym(self, name):
        return getattr(self._lib, self._prefix + name)

    def _call(self, entry, view, params, outputs):
        """view: None where the library takes its state from the parameters instead"""
        rc = self._sym(entry)(self._h, None if view is None else C.byref(view), C.byref(params), C.byref(outputs))
        if rc != 0:
            raise self._error(rc, self._sym('last_error')(self._h).decode())

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._sym('destroy')(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def last_kernel(self):
        return self._sym('last_kernel')(self._h).decode()

    @property
    def last_kernel_ms(self):
        """Device time of the last call's kernel alone, without the copies (HIP events), in ms"""
        return float(self._sym('last_kernel_ms')(self._h))
