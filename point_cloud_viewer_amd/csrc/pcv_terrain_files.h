// pcv_terrain_files.h — the terrain directory's format and the parameter rules, plain host code (pcv_terrain_files.cpp).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pcv_hip.h"
#include "pcv_terrain_dev.h"

// what pcv_terrain_check_params_host refuses; *why says which rule
int pcv_terrain_check_params(const pcv_terrain_params* p, std::string* why);
// the grid of checked parameters: M = R^T / |q|^2 written out, t, origin, resolution
PcvTerrainGrid pcv_terrain_grid(const pcv_terrain_params& p);
std::string pcv_terrain_tile_name(int32_t x, int32_t y);  // "x{:08}_y{:08}"
std::string pcv_terrain_f64_json(double v);               // fewest of 15 / 16 / 17 digits that round-trip; integral values with ".0"
// the whole of meta.json; the JSON is made nowhere else
std::string pcv_terrain_meta_json(const pcv_terrain_params& p, uint64_t num_tiles, const int32_t* positions);
// masks of a w x h window of set flags whose first vertex is (i0, j0); outside the window nothing is set
void pcv_terrain_quad_masks(int64_t i0, int64_t j0, uint32_t w, uint32_t h, const uint8_t* set, uint32_t* masks);
// one whole file, written anew; PCV_E_IO with *why naming the path
int pcv_terrain_write_file(const std::string& path, const void* data, size_t bytes, std::string* why);
