/* build_from_las.c — "a tile of survey data in, a product out", in plain C11 on top of the C ABI: a LAS 1.0 - 1.4
 * file is decoded and filtered on the device (pcv_las_load) and the device-resident planes go, unchanged, into one of the
 * builders. The call sequence of a non-Python host:
 *   pcv_las_header_host -> pcv_las_check_params_host -> pcv_las_load -> pcv_las_cloud_points / _attributes ->
 *     --octree     pcv_build_octree (PCV_BUILD_COMPUTE_BBOX) -> pcv_octree_write_dir
 *     --s2         pcv_s2_split_ex -> pcv_s2_write_dir                       (ECEF points: see --global-from-local)
 *     --terrain    pcv_aabb_reduce -> pcv_terrain_begin -> pcv_terrain_add_points -> pcv_terrain_finish -> pcv_terrain_write_dir
 *     --map-tiles  pcv_maptiles_begin -> pcv_maptiles_add_points -> pcv_maptiles_finish -> pcv_maptiles_write_dir   (ECEF)
 * No point array is held on the host.
 *
 *   build_from_las <in.las> (--octree DIR --resolution R | --s2 DIR [--level L] | --terrain DIR --resolution R | --map-tiles DIR --zoom Z)
 *                  [--classes 2,6,...] [--drop-withheld] [--color auto|rgb16|rgb8|intensity|R,G,B] [--attributes a,b|all]
 *                  [--global-from-local tx,ty,tz,qi,qj,qk,qw] [--info]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: build_from_las <in.las> (--octree DIR --resolution R | --s2 DIR [--level L] | --terrain DIR --resolution R | --map-tiles DIR --zoom Z)\n"
    "                      [--classes 2,6,...] [--drop-withheld] [--color auto|rgb16|rgb8|intensity|R,G,B] [--attributes a,b|all]\n"
    "                      [--global-from-local tx,ty,tz,qi,qj,qk,qw] [--info]\n"
    "  --octree DIR          an octree directory at --resolution metres (colour and intensity)\n"
    "  --s2 DIR              an S2 cell cloud split at --level (default 20) with the --attributes as extras; needs ECEF points\n"
    "  --terrain DIR         height and colour tiles at --resolution metres per vertex\n"
    "  --map-tiles DIR       z/x/y PNG tiles at --zoom (0 ..= 23); needs ECEF points\n"
    "  --resolution R        metres, above 0\n"
    "  --level L             the S2 split level, 0 ..= 30\n"
    "  --zoom Z              the zoom the points are drawn at\n"
    "  --classes             the classes to keep, 0 ..= 255 each (default: all)\n"
    "  --drop-withheld       drop the records flagged withheld\n"
    "  --color               auto (default): rgb16 or rgb8 by the file's largest channel value, intensity for a format without\n"
    "                        colour; or one of the rules; or a constant R,G,B\n"
    "  --attributes          the extras kept for --s2: names of DESIGN 9j's table, or all\n"
    "  --global-from-local   an isometry applied to every point: translation and unit quaternion\n"
    "  --info                print the header and the histograms counted on the device; alone, nothing is built\n";

static int usage(void) {
  fputs(kUsage, stderr);
  return 2;
}

static int parse_int(const char* arg, long lo, long hi, long* out) {
  char* end = NULL;
  const long v = strtol(arg, &end, 10);
  if (end == arg || *end || v < lo || v > hi) return 0;
  *out = v;
  return 1;
}
/* `count` comma-separated numbers */
static int parse_doubles(const char* s, int count, double* out) {
  for (int k = 0; k < count; ++k) {
    char* end = NULL;
    out[k] = strtod(s, &end);
    if (end == s || *end != (k + 1 < count ? ',' : '\0')) return 0;
    s = end + 1;
  }
  return 1;
}

enum { PRODUCT_NONE, PRODUCT_OCTREE, PRODUCT_S2, PRODUCT_TERRAIN, PRODUCT_MAP_TILES };

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (strcmp(argv[i], "--help") == 0 || strcmp(argv[i], "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    }
  const char *input = NULL, *output = NULL, *attributes = NULL;
  int product = PRODUCT_NONE, want_info = 0;
  double resolution = 0;
  long level = 20, zoom = -1;
  pcv_las_params lp;
  memset(&lp, 0, sizeof(lp));
  static char names[PCV_LAS_MAX_EXTRAS][32];
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    int p = strcmp(a, "--octree") == 0 ? PRODUCT_OCTREE : strcmp(a, "--s2") == 0 ? PRODUCT_S2 : strcmp(a, "--terrain") == 0 ? PRODUCT_TERRAIN
            : strcmp(a, "--map-tiles") == 0 ? PRODUCT_MAP_TILES : PRODUCT_NONE;
    if (p != PRODUCT_NONE) {
      if (!more || product != PRODUCT_NONE) return usage();
      product = p, output = argv[++i];
    } else if (strcmp(a, "--resolution") == 0 && more) {
      if (!parse_doubles(argv[++i], 1, &resolution) || !(resolution > 0)) return usage();
    } else if (strcmp(a, "--level") == 0 && more) {
      if (!parse_int(argv[++i], 0, 30, &level)) return usage();
    } else if (strcmp(a, "--zoom") == 0 && more) {
      if (!parse_int(argv[++i], 0, PCV_MAPTILES_MAX_ZOOM, &zoom)) return usage();
    } else if (strcmp(a, "--classes") == 0 && more) {
      const char* s = argv[++i];
      for (;;) {
        char* end = NULL;
        const long c = strtol(s, &end, 10);
        if (end == s || c < 0 || c > 255 || (*end != ',' && *end != '\0')) return usage();
        lp.class_mask[c >> 6] |= (uint64_t)1 << (c & 63);
        if (!*end) break;
        s = end + 1;
      }
    } else if (strcmp(a, "--drop-withheld") == 0) {
      lp.drop_withheld = 1;
    } else if (strcmp(a, "--color") == 0 && more) {
      const char* s = argv[++i];
      double c[3];
      if (strcmp(s, "auto") == 0) lp.color_mode = PCV_LAS_COLOR_AUTO;
      else if (strcmp(s, "rgb16") == 0) lp.color_mode = PCV_LAS_COLOR_RGB16;
      else if (strcmp(s, "rgb8") == 0) lp.color_mode = PCV_LAS_COLOR_RGB8;
      else if (strcmp(s, "intensity") == 0) lp.color_mode = PCV_LAS_COLOR_INTENSITY;
      else if (parse_doubles(s, 3, c) && c[0] >= 0 && c[0] <= 255 && c[1] >= 0 && c[1] <= 255 && c[2] >= 0 && c[2] <= 255) {
        lp.color_mode = PCV_LAS_COLOR_CONSTANT;
        for (int k = 0; k < 3; ++k) lp.constant_color[k] = (uint8_t)c[k];
      } else return usage();
    } else if (strcmp(a, "--attributes") == 0 && more) {
      attributes = argv[++i];
    } else if (strcmp(a, "--global-from-local") == 0 && more) {
      if (!parse_doubles(argv[++i], 7, lp.global_from_local)) return usage();
      lp.use_transform = 1;
    } else if (strcmp(a, "--info") == 0) {
      want_info = 1;
    } else if (a[0] != '-' && !input) {
      input = a;
    } else {
      return usage();
    }
  }
  if (!input || (product == PRODUCT_NONE && !want_info)) return usage();
  if ((product == PRODUCT_OCTREE || product == PRODUCT_TERRAIN) && !(resolution > 0)) return usage();
  if (product == PRODUCT_MAP_TILES && zoom < 0) return usage();

  pcv_las_header hdr;
  int rc;
  if ((rc = pcv_las_header_host(input, &hdr)) != PCV_OK) {
    fprintf(stderr, "cannot read %s (%d): %s\n", input, rc, pcv_host_last_error());
    return 1;
  }
  if (attributes && strcmp(attributes, "all") == 0) {
    pcv_las_extras_host(hdr.point_format, lp.extras, NULL, &lp.num_extras);
  } else if (attributes) {
    const char* s = attributes;
    while (*s) {
      const size_t len = strcspn(s, ",");
      if (len == 0 || len >= sizeof(names[0]) || lp.num_extras == PCV_LAS_MAX_EXTRAS) return usage();
      memcpy(names[lp.num_extras], s, len);
      lp.extras[lp.num_extras] = names[lp.num_extras];
      lp.num_extras += 1;
      s += len + (s[len] == ',');
    }
  }
  lp.keep_intensity = product == PRODUCT_OCTREE || product == PRODUCT_S2;
  if ((rc = pcv_las_check_params_host(&hdr, &lp)) != PCV_OK) {
    fprintf(stderr, "%s\n", pcv_host_last_error());
    return usage();
  }

  pcv_ctx* ctx = NULL;
  if ((rc = pcv_ctx_create(0, NULL, &ctx)) != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    return 1;
  }
  pcv_las_cloud* cloud = NULL;
  pcv_octree* tree = NULL;
  pcv_s2_cloud* cells = NULL;
  pcv_terrain* terrain = NULL;
  pcv_maptiles* tiles = NULL;
  const char* what = "load";
  if ((rc = pcv_las_load(ctx, input, &lp, &cloud)) != PCV_OK) goto done;
  pcv_las_info info;
  pcv_points pts;
  pcv_attribute attrs[PCV_LAS_MAX_EXTRAS];
  uint32_t num_attrs = 0;
  pcv_las_cloud_info(cloud, &info);
  pcv_las_cloud_points(cloud, &pts);
  pcv_las_cloud_attributes(cloud, &num_attrs, attrs);
  if (want_info) {
    static const char* const rules[] = {"auto", "rgb16", "rgb8", "intensity", "constant"};
    static const char* const flags[] = {"synthetic", "key-point", "withheld", "overlap"};
    printf("%s: LAS %u.%u, point data record format %u, %u bytes per record, %llu records at offset %u\n", input, hdr.version_major,
           hdr.version_minor, hdr.point_format, hdr.record_length, (unsigned long long)hdr.num_points, hdr.offset_to_points);
    printf("scale %.17g %.17g %.17g, offset %.17g %.17g %.17g\n", hdr.scale[0], hdr.scale[1], hdr.scale[2], hdr.offset[0], hdr.offset[1], hdr.offset[2]);
    printf("kept %llu, dropped by class %llu, dropped as withheld %llu, in %u pieces\n", (unsigned long long)info.num_kept,
           (unsigned long long)info.dropped_class, (unsigned long long)info.dropped_withheld, info.num_pieces);
    printf("largest colour channel %u, largest intensity %u, colour rule %s\n", info.max_color, info.max_intensity, rules[info.color_rule]);
    for (int c = 0; c < 256; ++c)
      if (info.class_hist[c]) printf("class %d: %llu\n", c, (unsigned long long)info.class_hist[c]);
    for (int r = 0; r < 16; ++r)
      if (info.return_hist[r]) printf("return %d: %llu\n", r, (unsigned long long)info.return_hist[r]);
    for (int b = 0; b < 4; ++b) printf("%s: %llu\n", flags[b], (unsigned long long)info.flag_counts[b]);
  }

  if (product == PRODUCT_OCTREE) {
    what = "octree";
    pcv_build_params bp;
    memset(&bp, 0, sizeof(bp));
    bp.resolution = resolution, bp.flags = PCV_BUILD_COMPUTE_BBOX;
    if ((rc = pcv_build_octree(ctx, &bp, &pts, &tree)) != PCV_OK) goto done;
    rc = pcv_octree_write_dir(tree, output);
  } else if (product == PRODUCT_S2) {
    what = "S2 cells";
    if ((rc = pcv_s2_split_ex(ctx, &pts, attrs, num_attrs, (uint32_t)level, &cells)) != PCV_OK) goto done;
    rc = pcv_s2_write_dir(cells, output);
  } else if (product == PRODUCT_TERRAIN) {
    what = "terrain";
    pcv_terrain_params tp;
    memset(&tp, 0, sizeof(tp));
    tp.tile_size = 256, tp.statistic = PCV_TERRAIN_MAX, tp.resolution_m = resolution, tp.world_from_terrain[6] = 1.0, tp.min_points = 1;
    double lo[3], hi[3];
    if ((rc = pcv_aabb_reduce(ctx, &pts, lo, hi)) != PCV_OK) goto done;
    if ((rc = pcv_terrain_begin(ctx, &tp, lo, hi, &terrain)) != PCV_OK) goto done;
    if ((rc = pcv_terrain_add_points(terrain, pts.n, pts.x, pts.y, pts.z, pts.color, PCV_MEM_DEVICE)) != PCV_OK) goto done;
    if ((rc = pcv_terrain_finish(terrain)) != PCV_OK) goto done;
    rc = pcv_terrain_write_dir(terrain, output);
  } else if (product == PRODUCT_MAP_TILES) {
    what = "map tiles";
    pcv_maptiles_params mp;
    memset(&mp, 0, sizeof(mp));
    mp.zoom = (uint32_t)zoom, mp.max_tiles = 1u << 20;
    if ((rc = pcv_maptiles_begin(ctx, &mp, &tiles)) != PCV_OK) goto done;
    if ((rc = pcv_maptiles_add_points(tiles, pts.n, pts.x, pts.y, pts.z, pts.color, PCV_MEM_DEVICE)) != PCV_OK) goto done;
    if ((rc = pcv_maptiles_finish(tiles)) != PCV_OK) goto done;
    rc = pcv_maptiles_write_dir(tiles, output, PCV_XRAY_PNG_STORED);
  }
  if (rc == PCV_OK && product != PRODUCT_NONE)
    printf("%s: %llu of %llu records -> %s\n", input, (unsigned long long)info.num_kept, (unsigned long long)info.num_records, output);

done:
  if (rc != PCV_OK) fprintf(stderr, "%s failed (%d): %s\n", what, rc, pcv_last_error(ctx));
  pcv_maptiles_free(tiles);
  pcv_terrain_free(terrain);
  if (cells) pcv_s2_free(cells);
  if (tree) pcv_octree_free(tree);
  pcv_las_cloud_free(cloud);
  pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
