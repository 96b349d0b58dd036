/* query_batch.c — xray-style tile queries over the C ABI in plain C11: an octree directory is opened, a tiles x tiles grid of
 * AABBs over its bounding box (x and y split evenly, z the whole box) goes to pcv_query_batch_run as one batch, and the
 * number of kept points of every tile is printed, one line "<i> <j> <count>" per tile, shape i * tiles + j. The points of
 * a tile would be copied out with pcv_query_batch_points over its segments.
 *
 *   query_batch <dir> <tiles>
 *   query_batch <dir> --map-tiles <zoom>
 *   query_batch <dir> --cells <token>[,<token>...]
 *
 * --map-tiles: the octree is an ECEF cloud; the slippy-map tiles of zoom level <zoom> (8..23: a WebMercatorRect is at most one
 * pixel of zoom 0 wide, i.e. one tile of zoom 8) that the projection of the bounding box's corners spans go to the batch as
 * PCV_SHAPE_WEB_MERCATOR_RECT shapes made by pcv_wmr_from_zoomed, row by row; one line "<tile x> <tile y> <count>" per tile.
 *
 * --cells: the octree is an ECEF cloud; the S2 cells given as tokens (CellID::to_token: the id's hex digits without trailing
 * zeros) are one cell union (PointLocation::S2Cells), sorted and handed to pcv_shapes_create_ex as the one shape of the batch;
 * one line "<nodes> <points>": the nodes the union's walk lists and the points it keeps.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static int by_id(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : (x > y ? 1 : 0);
}

/* one union from "<token>,<token>,...": ids ascending; NULL when a token is not 1..16 hex digits */
static uint64_t* cells_of_tokens(const char* list, uint32_t* count) {
  size_t n = 1;
  for (const char* p = list; *p; ++p) n += *p == ',';
  uint64_t* ids = (uint64_t*)calloc(n, sizeof(uint64_t));
  n = 0;
  for (const char* p = list; ids;) {
    uint64_t id = 0;
    int digits = 0;
    for (; *p && *p != ','; ++p, ++digits) {
      const int c = *p;
      const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (v < 0 || digits >= 16) {
        free(ids);
        return NULL;
      }
      id = (id << 4) | (uint64_t)v;
    }
    if (digits == 0) {
      free(ids);
      return NULL;
    }
    ids[n++] = id << (4 * (16 - digits));
    if (!*p) break;
    ++p;
  }
  qsort(ids, n, sizeof(uint64_t), by_id);
  *count = (uint32_t)n;
  return ids;
}

int main(int argc, char** argv) {
  const int map_tiles = argc >= 4 && strcmp(argv[2], "--map-tiles") == 0;
  const int by_cells = argc >= 4 && strcmp(argv[2], "--cells") == 0;
  if (argc < 3 || (argc >= 4 && !map_tiles && !by_cells)) {
    fprintf(stderr, "usage: query_batch <dir> <tiles> | query_batch <dir> --map-tiles <zoom> | query_batch <dir> --cells <token>[,<token>...]\n");
    return 2;
  }
  uint32_t union_first[2] = {0, 0};
  uint64_t* union_cells = by_cells ? cells_of_tokens(argv[3], &union_first[1]) : NULL;
  if (by_cells && !union_cells) {
    fprintf(stderr, "a token is 1..16 hex digits\n");
    return 2;
  }
  const unsigned tiles = map_tiles || by_cells ? 1u : (unsigned)strtoul(argv[2], NULL, 10);
  const unsigned zoom = map_tiles ? (unsigned)strtoul(argv[3], NULL, 10) : 0u;
  if (tiles == 0) {
    fprintf(stderr, "tiles must be positive\n");
    return 2;
  }
  if (map_tiles && (zoom < 8 || zoom > 23)) {
    fprintf(stderr, "zoom must be 8..23\n");
    return 2;
  }
  pcv_ctx* ctx = NULL;
  pcv_octree* tree = NULL;
  pcv_shapes* shapes = NULL;
  pcv_query_batch* batch = NULL;
  pcv_shape* grid = NULL;
  uint64_t* first = NULL;
  uint64_t* offset = NULL;
  int rc = pcv_ctx_create(0, NULL, &ctx);
  if (rc == PCV_OK) rc = pcv_octree_open_dir(ctx, argv[1], &tree);
  if (rc == PCV_OK) {
    double res, bmin[3], bmax[3];
    int version;
    pcv_octree_meta(tree, &res, bmin, bmax, &version);
    unsigned count = tiles * tiles;
    unsigned tx0 = 0, ty0 = 0, ntx = 0;
    if (map_tiles) { /* the tiles under the projection of the box's eight corners */
      double cx[8], cy[8], cz[8], u[8], v[8];
      for (int c = 0; c < 8; ++c) {
        cx[c] = (c & 1) ? bmax[0] : bmin[0];
        cy[c] = (c & 2) ? bmax[1] : bmin[1];
        cz[c] = (c & 4) ? bmax[2] : bmin[2];
      }
      rc = pcv_wmr_project(8, cx, cy, cz, u, v);
      double ulo = u[0], uhi = u[0], vlo = v[0], vhi = v[0];
      for (int c = 1; c < 8; ++c) {
        ulo = u[c] < ulo ? u[c] : ulo;
        uhi = u[c] > uhi ? u[c] : uhi;
        vlo = v[c] < vlo ? v[c] : vlo;
        vhi = v[c] > vhi ? v[c] : vhi;
      }
      const double n = (double)(1u << zoom);
      const unsigned last = (1u << zoom) - 1u;
      tx0 = (unsigned)(ulo * n);
      ty0 = (unsigned)(vlo * n);
      unsigned tx1 = (unsigned)(uhi * n), ty1 = (unsigned)(vhi * n);
      tx1 = tx1 > last ? last : tx1;
      ty1 = ty1 > last ? last : ty1;
      ntx = tx1 - tx0 + 1;
      if (rc == PCV_OK && (uint64_t)ntx * (ty1 - ty0 + 1) > (1u << 20)) {
        fprintf(stderr, "more than 2^20 tiles at this zoom\n");
        rc = PCV_E_INVALID;
      }
      count = rc == PCV_OK ? ntx * (ty1 - ty0 + 1) : 0;
    }
    grid = (pcv_shape*)calloc(count ? count : 1, sizeof(pcv_shape));
    for (unsigned k = 0; map_tiles && rc == PCV_OK && k < count; ++k) {
      /* a tile's south-east corner belongs to the next tile (contains() is half-open); the map's last row / column ends one
       * representable step inside the map, where from_zoomed still accepts it */
      const double px = 256.0 * (tx0 + k % ntx), py = 256.0 * (ty0 + k / ntx), edge = 256.0 * (double)(1u << zoom);
      const double mn[2] = {px, py};
      double mx[2] = {px + 256.0, py + 256.0};
      if (mx[0] >= edge) mx[0] = edge * (1.0 - 1.1102230246251565e-16);
      if (mx[1] >= edge) mx[1] = edge * (1.0 - 1.1102230246251565e-16);
      grid[k].kind = PCV_SHAPE_WEB_MERCATOR_RECT;
      rc = pcv_wmr_from_zoomed(mn, mx, zoom, grid[k].params);
    }
    if (by_cells) grid[0].kind = PCV_SHAPE_S2_CELL_UNION; /* .reserved = 0: the first (and only) union */
    for (unsigned i = 0; !map_tiles && !by_cells && rc == PCV_OK && i < tiles; ++i)
      for (unsigned j = 0; j < tiles; ++j) {
        pcv_shape* s = &grid[i * tiles + j];
        s->kind = PCV_SHAPE_AABB;
        s->params[0] = bmin[0] + (bmax[0] - bmin[0]) * i / tiles;
        s->params[1] = bmin[1] + (bmax[1] - bmin[1]) * j / tiles;
        s->params[2] = bmin[2];
        s->params[3] = bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / tiles;
        s->params[4] = bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / tiles;
        s->params[5] = bmax[2];
      }
    if (rc == PCV_OK)
      rc = by_cells ? pcv_shapes_create_ex(ctx, grid, count, 1, union_first, union_cells, &shapes) : pcv_shapes_create(ctx, grid, count, &shapes);
    if (rc == PCV_OK) rc = pcv_query_batch_run(ctx, shapes, tree, NULL, NULL, &batch);
    pcv_shapes_free(shapes); /* the batch does not need the shapes any more */
    uint64_t nseg = 0, npts = 0;
    if (rc == PCV_OK) rc = pcv_query_batch_sizes(batch, &nseg, &npts);
    if (rc == PCV_OK) {
      first = (uint64_t*)malloc(sizeof(uint64_t) * (count + 1));
      offset = (uint64_t*)malloc(sizeof(uint64_t) * (nseg + 1));
      rc = pcv_query_batch_segments(batch, first, NULL, offset);
    }
    if (rc == PCV_OK && by_cells) printf("%llu %llu\n", (unsigned long long)nseg, (unsigned long long)npts);
    for (unsigned k = 0; rc == PCV_OK && !by_cells && k < count; ++k)
      printf("%u %u %llu\n", map_tiles ? tx0 + k % ntx : k / tiles, map_tiles ? ty0 + k / ntx : k % tiles,
             (unsigned long long)(offset[first[k + 1]] - offset[first[k]]));
  }
  if (rc != PCV_OK) fprintf(stderr, "query_batch: %s (%d)\n", ctx ? pcv_last_error(ctx) : "no context", rc);
  free(first);
  free(offset);
  free(grid);
  free(union_cells);
  pcv_query_batch_free(batch);
  if (tree) pcv_octree_free(tree);
  if (ctx) pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
