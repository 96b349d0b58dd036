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
// the reader of that text (read_write.rs's serde schema): the five keys in any order, unknown keys skipped; fills tile_size,
// resolution_m, origin, world_from_terrain (the rest of *p: statistic MAX, min_points 1, default limits) and the tile
// positions, 2 per tile. PCV_E_INVALID with *why naming the key that is missing, of the wrong type or cut off.
int pcv_terrain_meta_read(const char* text, size_t len, pcv_terrain_params* p, std::vector<int32_t>* positions, std::string* why);
// one whole file of exactly `bytes` bytes; PCV_E_IO (cannot open / read) or PCV_E_INVALID (another length), *why names the path
int pcv_terrain_read_file(const std::string& path, void* data, size_t bytes, std::string* why);
// a whole file of any length (meta.json)
int pcv_terrain_read_text(const std::string& path, std::string* text, std::string* why);
// the window position of a camera, false when it is not representable
bool pcv_terrain_window_pos(const PcvTerrainGrid& g, const double c[3], uint32_t window, int64_t pos[2]);
// masks of a w x h window of set flags whose first vertex is (i0, j0); outside the window nothing is set
void pcv_terrain_quad_masks(int64_t i0, int64_t j0, uint32_t w, uint32_t h, const uint8_t* set, uint32_t* masks);
// one whole file, written anew; PCV_E_IO with *why naming the path
int pcv_terrain_write_file(const std::string& path, const void* data, size_t bytes, std::string* why);
