// Host-side descriptor helpers (see descriptor.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "common.hpp"

namespace pfa {

/// strides / distance / offset of one domain of a descriptor
struct view_t {
  std::vector<uint64_t> strides;
  int n_strides = 0;
  uint64_t distance = 0;
  uint64_t offset = 0;
};

std::vector<uint64_t> default_strides(const pfft_desc_t& d);
uint64_t flattened_length(const pfft_desc_t& d);
view_t view_of(const pfft_desc_t& d, int direction);
/// elements a buffer of domain `direction` must hold (descriptor::get_input_count)
uint64_t buffer_count(const pfft_desc_t& d, int direction);
int layout_of(const pfft_desc_t& d, int direction);
/// a REAL descriptor with PFFT_EXT_REAL_TRANSFORMS: forward domain in scalars, backward domain N/2 + 1 complex bins
bool is_real(const pfft_desc_t& d);
/// n has a prime factor above 61, the largest radix of any kernel: the ordinary planner refuses it
bool has_large_prime_factor(uint64_t n);
/// a descriptor with PFFT_EXT_ANY_LENGTH whose length the ordinary planner would refuse for its prime factor: planned
/// by plan_t::plan_bluestein (every other descriptor with the bit takes the ordinary path)
bool is_any_length(const pfft_desc_t& d);
/// a COMPLEX descriptor with PFFT_EXT_CONVOLUTION: the ordinary plan plus the fused convolution stages (plan_t::plan_conv)
bool has_convolution(const pfft_desc_t& d);
/// a REAL descriptor with PFFT_EXT_REAL_CONVOLUTION: the real plan plus the fused real convolution stages
/// (plan_t::plan_rconv); is_real holds for it too
bool has_real_convolution(const pfft_desc_t& d);
/// throws pfa::error(invalid / unsupported) like detail::validate::validate_descriptor
void validate(const pfft_desc_t& d);
int64_t largest_factor_le(int64_t n, int64_t limit);
bool fits_wavefront_registers(int64_t n, int scalar_bytes);
const std::string& last_error();

}  // namespace pfa
