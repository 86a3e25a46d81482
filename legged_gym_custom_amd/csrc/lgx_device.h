// lgx_device.h — small device helpers for the env-step kernels (gfx950, wave64): the DPP and
// readlane forms. The scalar math and the Philox RNG shared with the host backend are in
// lgx_env_common.h, included here for the kernels that only draw noise (lgx_act.hip, lgx_mlp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgx_env_common.h"

#define LGX_DEV __device__ __forceinline__

// ---------------------------------------------------------------- wave helpers
template <int CTRL>
LGX_DEV float dpp_shr_t(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// Sum over lanes 0..15 (DPP row 0), returned to every lane. Lanes 0..15 must be active;
// the other rows' values are ignored.
LGX_DEV float row0_sum16(float x) {
  x += dpp_shr_t<0x111>(x);
  x += dpp_shr_t<0x112>(x);
  x += dpp_shr_t<0x114>(x);
  x += dpp_shr_t<0x118>(x);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 15));
}

LGX_DEV int lane_id() { return __lane_id(); }
