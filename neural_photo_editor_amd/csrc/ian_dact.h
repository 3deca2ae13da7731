// ian_dact.h -- the activation derivative the backward kernels share: grad_pass and beta_bwd (kernels_misc.hip), the latent brush's
// seed and dec_out backward (kernels_brush.hip).  Include it BEFORE anything that changes the floating-point contraction mode:
// 1 - y*y is one fma under the default mode in every file.
#pragma once

namespace ian {

// derivative of the activation in terms of its OUTPUT y (enum ian_act)
__device__ __forceinline__ float m_dact(float y, int act) {
  switch (act) {
    case 1: return y > 0.f ? 1.f : 0.f;
    case 2: return y > 0.f ? 1.f : 0.2f;
    case 3: return y > 0.f ? 1.f : y + 1.f;
    case 4: return 1.f - y * y;
    case 5: return y * (1.f - y);
    default: return 1.f;
  }
}

}  // namespace ian
