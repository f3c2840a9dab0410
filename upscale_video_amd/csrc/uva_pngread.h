// uva_pngread.h -- the PNG reader and the inflate of csrc/uva_pngread.cpp (host only), as the uva_png_decode_* entries call them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace uva {
int png_read_bgr(const uint8_t* file, size_t len, uint8_t* out, size_t cap, int* h_out, int* w_out, std::string& err);
int png_read_bgr16(const uint8_t* file, size_t len, uint16_t* out, size_t cap, int* h_out, int* w_out, std::string& err);
int zlib_decompress_exact(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, std::string& err);
}  // namespace uva
