"""Per-block cycle account of lgx_s8_heads_fwd's tiles (dev tool, GPU) at the go2 minibatch shape
(24,576 rows, 256 -> 128 -> {12, 1}): a -DLGX_S8_CLOCK build of liblgx_s8 (build_native.build_variant)
given as LGX_S8_LIB; thread 0 of every block reports clock64 deltas of its phases (lgx_s8.hip,
s8_heads_fwd_kernel). The problem is tests/test_gpu_s8_heads_fwd.py's, at the production row count.
Usage: LGX_S8_LIB=<clock build> PYTHONPATH=.:tests python tools/heads_fwd_clock.py"""
import ctypes as C

import numpy as np
import torch

import test_gpu_s8_heads_fwd as T
from legged_gym_custom_amd.rsl_rl.modules import hip_s8 as S

M, HD, A = 24576, 128, 12
PHASES = ("K loop", "bias+ELU+y2 store", "last layer", "head rows", "level 0 + stores", "partials+colsums")


def main():
    L = S.lib()
    L.lgx_s8_set_clock.argtypes = [C.c_void_p]
    buf = torch.zeros(12 * 4096, dtype=torch.int32, device=T.dev)
    for _ in range(2):
        T._run(M, HD, A, fused=True)
    assert L.lgx_s8_set_clock(buf.data_ptr()) == 0
    T._run(M, HD, A, fused=True)
    L.lgx_s8_set_clock(None)
    d = buf.view(-1, 12).cpu().numpy().astype(np.int64)
    d = d[d[:, 6] > 0]
    for kind, name in ((1, "actor"), (2, "critic")):
        k = d[d[:, 7] == kind]
        print(f"{name} tiles: {len(k)} blocks, {int(k[:, 8].mean())} K steps, block total {k[:, 6].mean():8.0f} cycles "
              f"(p10 {np.percentile(k[:, 6], 10):8.0f}, max {k[:, 6].max():8.0f})")
        print("   " + "   ".join(f"{p} {k[:, q].mean():7.0f}" for q, p in enumerate(PHASES)))


if __name__ == "__main__":
    main()
