// ms_geometry.h -- the host geometry of the ORB front end (geometry.cpp): restates static_settings.cpp:9-60 and image_pyramid.cpp:76-78.
// Plain C++17, no HIP: ms_internal.h includes this header, and orb_geom.h and its check (tests/orb_geom_check.cpp) call geometry.cpp through it.
#pragma once
#include <cstdint>
#include <vector>

namespace msgeo {
void scale_factors(int levels, float f, float *out);
void level_sigma_sq(int levels, float f, float *out);
void level_quotas(int levels, float f, int max_kpts, int32_t *out);
void level_sizes(int levels, float f, int w0, int h0, int32_t *w, int32_t *h);
void umax(int32_t *u16);
// cv::resize INTER_LINEAR 8U coefficient tables (11-bit fixed point)
void resize_tables(int src_n, int dst_n, bool is_x, std::vector<int16_t> &ofs, std::vector<int16_t> &coef);
}  // namespace msgeo

inline int ms_div_up(int a, int b) { return (a + b - 1) / b; }
