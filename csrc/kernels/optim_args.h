// Operands of the single-segment optimiser launches (optim.hip aca_adam_step / aca_rmsprop_step), shared with
// csrc/bindings.cpp: plain C types only, so both hipcc and g++ compile this header. Host side only: the launcher
// builds the kernel's OptSeg from them.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace aca {

struct OptStepArgs {
  float* p; float* g;
  float* m;                   // Adam only
  float* v;
  size_t n;
  const float* lr;            // device scalar
  float* t;                   // Adam only: device step count
  const float* gnorm_parts;   // optional sumsq partials (global-norm clipping)
  float* gnorm_out;           // optional
  uint16_t* shadow;           // optional bf16 copy of p
  float b1;                   // Adam only
  float b2;                   // RMSprop: alpha
  float eps, clip, max_norm;
  unsigned int* ticket;       // Adam only
  int zero_grad;
  float gmul, norm_mul;
  const int64_t* trans;       // optional host table [8, 5] of weight copies written by the update (OptTrans)
  const uint16_t* g16;        // optional bf16 gradient read in place of g
};

}  // namespace aca
