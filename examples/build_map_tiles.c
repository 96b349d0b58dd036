/* build_map_tiles.c — "this cloud on a web map", in plain C11 on top of the C ABI: a z/x/y pyramid of 256-pixel PNG tiles
 * (the slippy-map layout) with tiles.json, from an ECEF octree directory or an S2 cell cloud directory (pcv_cloud_kind
 * decides). The reference has the tile coordinates (src/math/web_mercator.rs) and ships no generator; the product is stated
 * in include/pcv_hip.h. The call sequence of a non-Python host:
 *   pcv_cloud_kind -> pcv_octree_open_dir | pcv_s2_open_dir -> pcv_shapes_create (AllPoints) -> pcv_query_batch_run |
 *   pcv_s2_query_run -> pcv_maptiles_begin -> pcv_maptiles_add_query_batch | pcv_maptiles_add_s2_query ->
 *   pcv_maptiles_finish -> pcv_maptiles_build_parents -> pcv_maptiles_write_dir
 * The points go from the query's tables into the tiles on the device, piece by piece: no point array is held on the host.
 *
 *   build_map_tiles <cloud dir> --output-directory D --zoom Z [--min-zoom A] [--png stored|deflate] [--background r,g,b,a]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: build_map_tiles <cloud dir> --output-directory D --zoom Z [--min-zoom A] [--png stored|deflate] [--background r,g,b,a]\n"
    "  <cloud dir>           an octree directory or an S2 cell cloud directory of ECEF points (meta.pb decides)\n"
    "  --output-directory    where <z>/<x>/<y>.png and tiles.json go\n"
    "  --zoom                the zoom the points are drawn at, 0 ..= 23\n"
    "  --min-zoom            the parent levels are built down to this zoom (default: --zoom, no parents)\n"
    "  --png                 stored (default) or deflate: run-length deflate, encoded on the device\n"
    "  --background          the colour of pixels without a point, four values 0 ..= 255 (default 0,0,0,0: transparent)\n";

static int usage(void) {
  fputs(kUsage, stderr);
  return 2;
}

/* a whole number in [lo, hi] */
static int parse_int(const char* arg, long lo, long hi, long* out) {
  char* end = NULL;
  const long v = strtol(arg, &end, 10);
  if (end == arg || *end || v < lo || v > hi) return 0;
  *out = v;
  return 1;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (strcmp(argv[i], "--help") == 0 || strcmp(argv[i], "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    }
  const char *dir = NULL, *output = NULL;
  pcv_maptiles_params params;
  memset(&params, 0, sizeof(params));
  params.max_tiles = 1u << 20;
  long zoom = -1, min_zoom = -1;
  int mode = PCV_XRAY_PNG_STORED;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    if (strcmp(a, "--output-directory") == 0 && more && !output) {
      output = argv[++i];
    } else if (strcmp(a, "--zoom") == 0 && more) {
      if (!parse_int(argv[++i], 0, PCV_MAPTILES_MAX_ZOOM, &zoom)) return usage();
    } else if (strcmp(a, "--min-zoom") == 0 && more) {
      if (!parse_int(argv[++i], 0, PCV_MAPTILES_MAX_ZOOM, &min_zoom)) return usage();
    } else if (strcmp(a, "--png") == 0 && more) {
      const char* s = argv[++i];
      if (strcmp(s, "stored") == 0) mode = PCV_XRAY_PNG_STORED;
      else if (strcmp(s, "deflate") == 0) mode = PCV_XRAY_PNG_DEFLATE;
      else return usage();
    } else if (strcmp(a, "--background") == 0 && more) {
      const char* s = argv[++i];
      params.background = 0;
      for (int k = 0; k < 4; ++k) {
        char* end = NULL;
        const long v = strtol(s, &end, 10);
        if (end == s || *end != (k < 3 ? ',' : '\0') || v < 0 || v > 255) return usage();
        params.background |= (uint32_t)v << (8 * k);
        s = end + 1;
      }
    } else if (a[0] != '-' && !dir) {
      dir = a;
    } else {
      return usage();
    }
  }
  if (!dir || !output || zoom < 0) return usage();
  if (min_zoom < 0) min_zoom = zoom;
  params.zoom = (uint32_t)zoom;
  if (pcv_maptiles_check_params_host(&params, (uint32_t)min_zoom) != PCV_OK) {
    fprintf(stderr, "%s\n", pcv_host_last_error());
    return usage();
  }

  int kind = 0, rc;
  if ((rc = pcv_cloud_kind(dir, &kind)) != PCV_OK) {
    fprintf(stderr, "cannot open %s (%d): %s\n", dir, rc, pcv_host_last_error());
    return 1;
  }
  pcv_ctx* ctx = NULL;
  if ((rc = pcv_ctx_create(0, NULL, &ctx)) != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    return 1;
  }
  pcv_octree* tree = NULL;
  pcv_s2_cloud* cloud = NULL;
  pcv_shapes* shapes = NULL;
  pcv_query_batch* batch = NULL;
  pcv_s2_query* query = NULL;
  pcv_maptiles* tiles = NULL;
  const char* what = "open";
  rc = kind == PCV_CLOUD_S2 ? pcv_s2_open_dir(ctx, dir, &cloud) : pcv_octree_open_dir(ctx, dir, &tree);
  if (rc != PCV_OK) goto done;

  what = "query";
  pcv_shape all;
  memset(&all, 0, sizeof(all));
  all.kind = PCV_SHAPE_ALL;
  uint64_t num_segments = 0, num_points = 0;
  if ((rc = pcv_shapes_create(ctx, &all, 1, &shapes)) != PCV_OK) goto done;
  if (cloud) {
    rc = pcv_s2_query_run(cloud, shapes, 0, NULL, NULL, NULL, NULL, &query);
    if (rc == PCV_OK) rc = pcv_s2_query_sizes(query, &num_segments, &num_points);
  } else {
    rc = pcv_query_batch_run(ctx, shapes, tree, NULL, NULL, &batch);
    if (rc == PCV_OK) rc = pcv_query_batch_sizes(batch, &num_segments, &num_points);
  }
  if (rc != PCV_OK) goto done;

  what = "map tiles";
  if ((rc = pcv_maptiles_begin(ctx, &params, &tiles)) != PCV_OK) goto done;
  rc = cloud ? pcv_maptiles_add_s2_query(tiles, query, 0, num_segments) : pcv_maptiles_add_query_batch(tiles, batch, 0, num_segments);
  if (rc == PCV_OK) rc = pcv_maptiles_finish(tiles);
  if (rc == PCV_OK) rc = pcv_maptiles_build_parents(tiles, (uint32_t)min_zoom);
  if (rc != PCV_OK) goto done;
  what = "write";
  if ((rc = pcv_maptiles_write_dir(tiles, output, mode)) != PCV_OK) goto done;
  pcv_maptiles_info info;
  pcv_maptiles_info_get(tiles, &info);
  unsigned long long total = 0;
  for (long z = min_zoom; z <= zoom; ++z) total += (unsigned long long)info.tiles[z];
  printf("%s: %llu points (%llu dropped), %llu tiles at zoom %ld, %llu tiles in zooms %ld ..= %ld -> %s\n", dir, (unsigned long long)info.points_added,
         (unsigned long long)info.dropped, (unsigned long long)info.tiles[zoom], zoom, total, min_zoom, zoom, output);

done:
  if (rc != PCV_OK) fprintf(stderr, "%s failed (%d): %s\n", what, rc, pcv_last_error(ctx));
  pcv_maptiles_free(tiles);
  pcv_query_batch_free(batch);
  if (query) pcv_s2_query_free(query);
  if (shapes) pcv_shapes_free(shapes);
  if (tree) pcv_octree_free(tree);
  if (cloud) pcv_s2_free(cloud);
  pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
