"""ctypes binding of tests/devgpu/libplume_devgpu.so: the unit-test lane bodies (tests/devsim/lane_ops.h) compiled for gfx950, one lane per element (test-only).
The same Python surface as tests/_devsim.py offers for these functions -- the marshalling IS _devsim's (Lanes), with this library and the dg_ prefix.  The library is
built by __graft_entry__.build() (make -C tests/devgpu; no GPU needed); it is never compiled from here: a missing library is an error.
After any non-zero return the binding raises and is POISONED: every later call raises at once, before it touches the GPU -- nothing more is started on a device that
has just reported an error."""
import ctypes as C
from pathlib import Path

from tests import _devsim

ROOT = Path(__file__).resolve().parent.parent
_SO = ROOT / "tests" / "devgpu" / "libplume_devgpu.so"
_lib = None
_poisoned = None


class DevGpuError(RuntimeError):
    pass


def lib():
    global _lib
    if _poisoned is not None:
        raise DevGpuError(f"the GPU lane harness is poisoned by an earlier failure, nothing more runs on the GPU: {_poisoned}")
    if _lib is None:
        if not _SO.exists():
            raise DevGpuError(f"{_SO} is missing: run __graft_entry__.build() (make -C tests/devgpu)")
        _lib = C.CDLL(str(_SO))
        _lib.dg_last_error.restype = C.c_char_p
    return _lib


def _failed(name, rc):
    global _poisoned
    text = (_lib.dg_last_error() or b"").decode(errors="replace") if _lib is not None else ""
    _poisoned = f"{name} returned {rc}: {text}"
    raise DevGpuError(_poisoned)


def poisoned():
    return _poisoned


GPU = _devsim.Lanes(lib, "dg_", _failed)
fe_op, fe_raw, group_raw, sc_op, glv, sha256 = GPU.fe_op, GPU.fe_raw, GPU.group_raw, GPU.sc_op, GPU.glv, GPU.sha256
eisd_entries, eis_half_gcd, eis_consistent = GPU.eisd_entries, GPU.eis_half_gcd, GPU.eis_consistent
h2c_op, rfc6979 = GPU.h2c_op, GPU.rfc6979
