// Device functions shared by the MFMA simulators (qsim_mfma.hip: 8 qubits, qsim12_mfma.hip: 12): a layer's gates as
// Kronecker blocks of 4 qubits, and the fp16 hi / lo split that carries fp32 values through the fp16 MFMA.
#pragma once
#include "qsim_gates.h"

namespace qd {
namespace qmdev {

typedef __attribute__((ext_vector_type(8))) _Float16 h8;
typedef __attribute__((ext_vector_type(4))) float f4;

constexpr float LO_SCALE = 2048.f, LO_INV = 1.f / 2048.f;

// R = RZ(phi) RY(theta): [[c e^-ip, -s e^-ip], [s e^ip, c e^ip]] (p = phi / 2), gate_fwd's matrix; entry [a][b] from
// t = (cos, sin) of theta / 2 and of phi / 2
__device__ __forceinline__ cf rot(float4 t, int a, int b) {
  const float m = (a == b) ? t.x : (a == 0 ? -t.y : t.y);
  return a == 0 ? cf{m * t.z, -m * t.w} : cf{m * t.z, m * t.w};
}
// (R_{q0+3} (x) .. (x) R_{q0})[a][b], 4-bit row / column
__device__ __forceinline__ cf kron4(const float4* tr, int q0, int a, int b) {
  cf v = {1.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) v = cmul(v, rot(tr[q0 + i], (a >> i) & 1, (b >> i) & 1));
  return v;
}
__device__ __forceinline__ void split(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)((v - (float)hi) * LO_SCALE);
}
__device__ __forceinline__ f4 mfma(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

}  // namespace qmdev
}  // namespace qd
