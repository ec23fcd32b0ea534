// What bindings.cpp and net_bindings.cpp share: the current stream, raw-address casts and the
// `sample` list both the trunk and the optimizer launch take.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "include/dqn_nets_k.h"

namespace {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

template <class T>
T P(int64_t v) { return reinterpret_cast<T>(static_cast<intptr_t>(v)); }

// the 16 pointers heading a `sample` list, in TrunkSample order (the caller checked its length and
// sets B and ninst); `who` names the caller in the error
inline dqn::TrunkSample trunk_sample(const std::vector<int64_t>& v, const char* who) {
  for (int i = 0; i < 16; ++i) TORCH_CHECK(v[i] != 0, who, " sample: null pointer");
  return dqn::TrunkSample{P<const int32_t*>(v[0]), P<int64_t*>(v[1]), P<int32_t*>(v[2]), P<const int32_t*>(v[3]),
                          P<const int32_t*>(v[4]), P<const int32_t*>(v[5]), P<const float*>(v[6]),
                          P<const float*>(v[7]), P<const float*>(v[8]), P<int32_t*>(v[9]), P<int32_t*>(v[10]),
                          P<float*>(v[11]), P<float*>(v[12]), P<float*>(v[13]), P<int32_t*>(v[14]),
                          P<int32_t*>(v[15]), 0, 0};
}

}  // namespace
