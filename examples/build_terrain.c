/* build_terrain.c — "the surface under this cloud", in plain C11 on top of the C ABI: a terrain layer directory as
 * `sdl_viewer --terrain <dir>` reads it (sdl_viewer/src/terrain_drawer/read_write.rs), from an octree directory or an S2 cell
 * cloud directory (pcv_cloud_kind decides). The reference ships the reader only; the reduction is stated in include/pcv_hip.h.
 * The call sequence of a non-Python host:
 *   pcv_cloud_kind -> pcv_octree_open_dir | pcv_s2_open_dir -> pcv_shapes_create (AllPoints) -> pcv_query_batch_run |
 *   pcv_s2_query_run -> pcv_terrain_begin -> pcv_terrain_add_query_batch | pcv_terrain_add_s2_query -> pcv_terrain_finish ->
 *   pcv_terrain_write_dir
 * The points go from the query's tables into the grid on the device, piece by piece: no point array is held on the host.
 *
 *   build_terrain <cloud dir> --output-directory D --resolution R [--tile-size T] [--statistic max|min|mean] [--min-points N]
 *                 [--terrain-from-world tx,ty,tz,qi,qj,qk,qw] [--origin x,y,z]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: build_terrain <cloud dir> --output-directory D --resolution R [--tile-size T] [--statistic max|min|mean]\n"
    "                     [--min-points N] [--terrain-from-world tx,ty,tz,qi,qj,qk,qw] [--origin x,y,z]\n"
    "  <cloud dir>           an octree directory or an S2 cell cloud directory (meta.pb decides)\n"
    "  --output-directory    where meta.json and the tiles' x########_y########.height / .color files go\n"
    "  --resolution          metres between grid vertices, > 0\n"
    "  --tile-size           vertices per tile edge, 1 ..= 4096 (default 256)\n"
    "  --statistic           what a vertex keeps of its points: the highest (max, default), the lowest, or the mean\n"
    "  --min-points          points a vertex needs to be set (default 1)\n"
    "  --terrain-from-world  the isometry into the terrain frame: translation, then unit quaternion ijkw (default: identity)\n"
    "  --origin              the grid origin in the terrain frame (default 0,0,0)\n";

static int usage(void) {
  fputs(kUsage, stderr);
  return 2;
}

/* exactly n comma-separated numbers */
static int parse_numbers(const char* arg, double* out, int n) {
  for (int k = 0; k < n; ++k) {
    char* end = NULL;
    out[k] = strtod(arg, &end);
    if (end == arg || *end != (k + 1 < n ? ',' : '\0')) return 0;
    arg = end + 1;
  }
  return 1;
}

/* v rotated by the unit quaternion q = ijkw */
static void rotate(const double q[4], const double v[3], double out[3]) {
  const double i = q[0], j = q[1], k = q[2], w = q[3];
  const double tx = 2 * (j * v[2] - k * v[1]), ty = 2 * (k * v[0] - i * v[2]), tz = 2 * (i * v[1] - j * v[0]);
  out[0] = v[0] + w * tx + (j * tz - k * ty);
  out[1] = v[1] + w * ty + (k * tx - i * tz);
  out[2] = v[2] + w * tz + (i * ty - j * tx);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (strcmp(argv[i], "--help") == 0 || strcmp(argv[i], "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    }
  const char *dir = NULL, *output = NULL;
  pcv_terrain_params params;
  memset(&params, 0, sizeof(params));
  params.tile_size = 256, params.statistic = PCV_TERRAIN_MAX, params.min_points = 1;
  params.world_from_terrain[6] = 1.0;
  int have_resolution = 0;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    char* end = NULL;
    if (strcmp(a, "--output-directory") == 0 && more && !output) {
      output = argv[++i];
    } else if (strcmp(a, "--resolution") == 0 && more) {
      params.resolution_m = strtod(argv[++i], &end);
      if (*end || end == argv[i]) return usage();
      have_resolution = 1;
    } else if (strcmp(a, "--tile-size") == 0 && more) {
      const long v = strtol(argv[++i], &end, 10);
      if (*end || end == argv[i] || v < 1 || v > 4096) return usage();
      params.tile_size = (uint32_t)v;
    } else if (strcmp(a, "--min-points") == 0 && more) {
      const long v = strtol(argv[++i], &end, 10);
      if (*end || end == argv[i] || v < 1 || v > 0x7fffffffl) return usage();
      params.min_points = (uint32_t)v;
    } else if (strcmp(a, "--statistic") == 0 && more) {
      const char* s = argv[++i];
      if (strcmp(s, "max") == 0) params.statistic = PCV_TERRAIN_MAX;
      else if (strcmp(s, "min") == 0) params.statistic = PCV_TERRAIN_MIN;
      else if (strcmp(s, "mean") == 0) params.statistic = PCV_TERRAIN_MEAN;
      else return usage();
    } else if (strcmp(a, "--terrain-from-world") == 0 && more) {
      /* the library takes world_from_terrain: the inverse, (-(q* t), q*) */
      double tfw[7], back[3];
      if (!parse_numbers(argv[++i], tfw, 7)) return usage();
      const double conj[4] = {-tfw[3], -tfw[4], -tfw[5], tfw[6]};
      rotate(conj, tfw, back);
      for (int k = 0; k < 3; ++k) params.world_from_terrain[k] = -back[k];
      memcpy(params.world_from_terrain + 3, conj, sizeof(conj));
    } else if (strcmp(a, "--origin") == 0 && more) {
      if (!parse_numbers(argv[++i], params.origin, 3)) return usage();
    } else if (a[0] != '-' && !dir) {
      dir = a;
    } else {
      return usage();
    }
  }
  if (!dir || !output || !have_resolution) return usage();
  if (pcv_terrain_check_params_host(&params) != PCV_OK) {
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
  pcv_terrain* terrain = NULL;
  double lo[3], hi[3];
  const char* what = "open";
  rc = kind == PCV_CLOUD_S2 ? pcv_s2_open_dir(ctx, dir, &cloud) : pcv_octree_open_dir(ctx, dir, &tree);
  if (rc != PCV_OK) goto done;
  if (cloud) pcv_s2_info(cloud, NULL, NULL, lo, hi, NULL, NULL);
  else pcv_octree_meta(tree, NULL, lo, hi, NULL);

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

  what = "terrain";
  if ((rc = pcv_terrain_begin(ctx, &params, lo, hi, &terrain)) != PCV_OK) goto done;
  rc = cloud ? pcv_terrain_add_s2_query(terrain, query, 0, num_segments) : pcv_terrain_add_query_batch(terrain, batch, 0, num_segments);
  if (rc == PCV_OK) rc = pcv_terrain_finish(terrain);
  if (rc != PCV_OK) goto done;
  what = "write";
  if ((rc = pcv_terrain_write_dir(terrain, output)) != PCV_OK) goto done;
  pcv_terrain_info info;
  pcv_terrain_info_get(terrain, &info);
  printf("%s: %llu points (%llu outside), %llu vertices set, %llu quads, %llu tiles of %u x %u -> %s\n", dir, (unsigned long long)info.points_added,
         (unsigned long long)info.outside, (unsigned long long)info.set_vertices, (unsigned long long)info.rendered_quads,
         (unsigned long long)info.tiles, params.tile_size, params.tile_size, output);

done:
  if (rc != PCV_OK) fprintf(stderr, "%s failed (%d): %s\n", what, rc, pcv_last_error(ctx));
  pcv_terrain_free(terrain);
  pcv_query_batch_free(batch);
  if (query) pcv_s2_query_free(query);
  if (shapes) pcv_shapes_free(shapes);
  if (tree) pcv_octree_free(tree);
  if (cloud) pcv_s2_free(cloud);
  pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
