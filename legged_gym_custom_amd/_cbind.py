"""The one ctypes loader of the native libraries (liblgx.so, liblgx_mlp.so, liblgx_s8.so).

Each header has one mirror module (_abi.py: lgx.h, _abi_mlp.py: lgx_mlp.h, rsl_rl/modules/hip_s8.py:
lgx_s8.h) that states three tables, and tests/test_abi.py compares all three with the compiled header:
  SIGNATURES  {export: (restype, (argtypes...))}   every function the header declares
  STRUCTS     {C typedef name: ctypes class}       every struct the header defines
  CONSTANTS   {C macro or enumerator: value}       every integer the package mirrors
`load` sets SIGNATURES on the CDLL's own function objects and returns the CDLL: a call goes
straight into ctypes, with no Python wrapper around it."""
import ctypes as C
import os

import torch


def load(path, name, signatures, structs, abi, sizeof, error):
    """Open library `name` (e.g. "liblgx_mlp") at `path` and check it against its mirror.
    abi: (version export, expected version); sizeof: {sizeof export: C typedef name in structs};
    error: the exception class to raise."""
    if not os.path.exists(path):
        raise error(f"{name}.so not built ({path}); run `python -m legged_gym_custom_amd.build_native`")
    L = C.CDLL(path)
    for fn, (restype, argtypes) in signatures.items():
        try:
            f = getattr(L, fn)
        except AttributeError:
            raise error(f"{name}.so does not export {fn}; rebuild") from None
        f.restype, f.argtypes = restype, argtypes
    if getattr(L, abi[0])() != abi[1]:
        raise error(f"{name} ABI version mismatch; rebuild")
    for fn, ctype in sizeof.items():
        n, want = getattr(L, fn)(), C.sizeof(structs[ctype])
        if n != want:
            raise error(f"{ctype} layout mismatch: C {n} vs ctypes {want}")
    return L


def stream():
    """The current HIP stream as the `void* stream` argument of a launch."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()
