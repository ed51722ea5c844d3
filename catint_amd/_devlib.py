"""What the ctypes bindings of the libraries that read a ``pnp_device_view`` (``_observe.py``, ``_balance.py``, ``_regrid.py``) share: the view's mirror,
loading a library with its five lifecycle symbols and its entry point, and the handle class."""
import ctypes as C
import os

EINVAL, ENOMEM, EDEVICE = -1, -2, -3
_PD = C.POINTER(C.c_double)


class PnpDeviceView(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('method', C.c_int32), ('nspecies', C.c_int32), ('nx', C.c_int32), ('row_pitch', C.c_int32),
                ('reserved', C.c_int32), ('batch', C.c_int64), ('c_dev', C.c_void_p), ('phi_dev', C.c_void_p), ('status_dev', C.c_void_p),
                ('stream', C.c_void_p)]


def _dptr(a):
    return a.ctypes.data_as(_PD) if a is not None else None


def symbols(prefix, entry):
    """Every symbol the library's header declares"""
    return [prefix + n for n in ('create', 'destroy', 'last_error', 'last_kernel', 'last_kernel_ms', entry)]


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
