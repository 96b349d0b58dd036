/* query_batch.c — xray-style tile queries over the C ABI in plain C11: an octree directory is opened, a tiles x tiles grid of
 * AABBs over its bounding box (x and y split evenly, z the whole box) goes to pcv_query_batch_run as one batch, and the
 * number of kept points of every tile is printed, one line "<i> <j> <count>" per tile, shape i * tiles + j. The points of
 * a tile would be copied out with pcv_query_batch_points over its segments.
 *
 *   query_batch <dir> <tiles>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: query_batch <dir> <tiles>\n");
    return 2;
  }
  const unsigned tiles = (unsigned)strtoul(argv[2], NULL, 10);
  if (tiles == 0) {
    fprintf(stderr, "tiles must be positive\n");
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
    const unsigned count = tiles * tiles;
    grid = (pcv_shape*)calloc(count, sizeof(pcv_shape));
    for (unsigned i = 0; rc == PCV_OK && i < tiles; ++i)
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
    if (rc == PCV_OK) rc = pcv_shapes_create(ctx, grid, count, &shapes);
    if (rc == PCV_OK) rc = pcv_query_batch_run(ctx, shapes, tree, NULL, NULL, &batch);
    pcv_shapes_free(shapes); /* the batch does not need the shapes any more */
    uint64_t nseg = 0, npts = 0;
    if (rc == PCV_OK) rc = pcv_query_batch_sizes(batch, &nseg, &npts);
    if (rc == PCV_OK) {
      first = (uint64_t*)malloc(sizeof(uint64_t) * (count + 1));
      offset = (uint64_t*)malloc(sizeof(uint64_t) * (nseg + 1));
      rc = pcv_query_batch_segments(batch, first, NULL, offset);
    }
    for (unsigned k = 0; rc == PCV_OK && k < count; ++k)
      printf("%u %u %llu\n", k / tiles, k % tiles, (unsigned long long)(offset[first[k + 1]] - offset[first[k]]));
  }
  if (rc != PCV_OK) fprintf(stderr, "query_batch: %s (%d)\n", ctx ? pcv_last_error(ctx) : "no context", rc);
  free(first);
  free(offset);
  free(grid);
  pcv_query_batch_free(batch);
  if (tree) pcv_octree_free(tree);
  if (ctx) pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
