/* build_xray_quadtree.c — xray's build_xray_quadtree over the C ABI in plain C11: one or more point cloud directories (the
 * reference's point_cloud_locations) are opened — all as octrees, or all as S2 cell clouds when the first directory's
 * meta.pb says so (pcv_cloud_kind, as PointCloudClientBuilder::build decides) — the leaf tiles over all of them are
 * rasterised on the device (pcv_xray_run_ex, or pcv_s2_open_dir + pcv_xray_run_s2_ex; over S2 directories --filter-interval,
 * repeatable, and --binning take any scalar attribute of the clouds, over octrees intensity alone),
 * every level above them up to the root node is built on the device (pcv_xray_build_parents), and
 * the quadtree directory the xray viewer loads is written: one <node>.png per node and the meta file
 * (pcv_xray_write_dir_ex). A subset of the reference binary's flags, and --png: stored (the default) or deflate, the
 * tiles compressed on the device. With --inpaint-distance-px the leaves are built with the transparent background,
 * inpainted on the device (pcv_xray_inpaint; the fill is not the reference's texture synthesis) and given
 * --tile-background-color afterwards: build_xray_quadtree and inpaint_xray_quadtree in one run, no directory between.
 *
 *   build_xray_quadtree <octree dir | S2 cell cloud dir>... --output-directory <dir> --resolution <m per px> [--tile-size <px>]
 *                       [--coloring-strategy xray|colored|colored_with_intensity|colored_with_height_stddev]
 *                       [--min-intensity <f>] [--max-intensity <f>] [--binning <attribute>=<size>] [--max-stddev <m>]
 *                       [--colormap jet|purplish] [--tile-background-color white|transparent]
 *                       [--filter-interval <attribute>=<lo>,<hi>]... [--root-node-id <r...>] [--png stored|deflate]
 *                       [--inpaint-distance-px <0..254>]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static int usage(void) {
  fprintf(stderr,
          "usage: build_xray_quadtree <octree dir | S2 cell cloud dir>... --output-directory <dir> --resolution <m per px>\n"
          "       [--tile-size <px>]\n"
          "       [--coloring-strategy xray|colored|colored_with_intensity|colored_with_height_stddev] [--min-intensity <f>]\n"
          "       [--max-intensity <f>] [--binning <attribute>=<size>] [--max-stddev <m>] [--colormap jet|purplish]\n"
          "       [--tile-background-color white|transparent] [--filter-interval <attribute>=<lo>,<hi>]... [--root-node-id <r...>]\n"
          "       [--png stored|deflate] [--inpaint-distance-px <0..254>]\n"
          "       attributes: any scalar one of S2 cell clouds (timestamp=30000000000), intensity alone with octrees\n"
          "       the first directory's meta.pb decides: octrees, or S2 directories (S2 cell clouds); all are opened as that kind\n");
  return 2;
}

int main(int argc, char** argv) {
  const char** inputs = (const char**)calloc((size_t)argc, sizeof(const char*));
  uint32_t num_inputs = 0;
  const char* output = NULL;
  const char* root = "r";
  int png = PCV_XRAY_PNG_STORED;
  long inpaint = -1; /* no inpainting */
  /* one entry per --filter-interval; the names are copies that live until the run is over */
  pcv_xray_filter* filters = (pcv_xray_filter*)calloc((size_t)argc, sizeof(pcv_xray_filter));
  char** filter_names = (char**)calloc((size_t)argc, sizeof(char*));
  uint32_t num_filters = 0;
  char bin_attribute[PCV_S2_MAX_ATTR_NAME + 1] = "";
  pcv_xray_coloring col;
  memset(&col, 0, sizeof(col));
  col.min_intensity = 0.0f; /* the reference's defaults (build_quadtree.rs:49-66) */
  col.max_intensity = 1.0f;
  pcv_xray_params p;
  memset(&p, 0, sizeof(p));
  p.tile_size_px = 256;
  p.strategy = PCV_XRAY_XRAY;
  p.max_stddev = 1.0f;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : NULL;
    if (a[0] != '-') {
      inputs[num_inputs++] = a;
      continue;
    }
    if (!v) return usage();
    ++i;
    if (!strcmp(a, "--output-directory")) {
      output = v;
    } else if (!strcmp(a, "--resolution")) {
      p.pixel_size_m = strtod(v, NULL);
    } else if (!strcmp(a, "--tile-size")) {
      p.tile_size_px = (uint32_t)strtoul(v, NULL, 10);
    } else if (!strcmp(a, "--coloring-strategy")) {
      if (!strcmp(v, "xray")) p.strategy = PCV_XRAY_XRAY;
      else if (!strcmp(v, "colored")) p.strategy = PCV_XRAY_COLORED;
      else if (!strcmp(v, "colored_with_intensity")) p.strategy = PCV_XRAY_COLORED_WITH_INTENSITY;
      else if (!strcmp(v, "colored_with_height_stddev")) p.strategy = PCV_XRAY_HEIGHT_STDDEV;
      else return usage();
    } else if (!strcmp(a, "--min-intensity")) {
      col.min_intensity = strtof(v, NULL);
    } else if (!strcmp(a, "--max-intensity")) {
      col.max_intensity = strtof(v, NULL);
    } else if (!strcmp(a, "--binning")) {
      const char* eq = strchr(v, '=');
      if (!eq || (size_t)(eq - v) >= sizeof(bin_attribute)) return usage();
      memcpy(bin_attribute, v, (size_t)(eq - v));
      bin_attribute[eq - v] = '\0';
      col.binning_attribute = bin_attribute;
      col.bin_size = strtod(eq + 1, NULL);
    } else if (!strcmp(a, "--max-stddev")) {
      p.max_stddev = strtof(v, NULL);
    } else if (!strcmp(a, "--colormap")) {
      if (!strcmp(v, "jet")) p.colormap = PCV_XRAY_JET;
      else if (!strcmp(v, "purplish")) p.colormap = PCV_XRAY_PURPLISH;
      else return usage();
    } else if (!strcmp(a, "--tile-background-color")) {
      if (!strcmp(v, "white")) p.background = PCV_XRAY_BG_WHITE;
      else if (!strcmp(v, "transparent")) p.background = PCV_XRAY_BG_TRANSPARENT;
      else return usage();
    } else if (!strcmp(a, "--filter-interval")) {
      const char* eq = strchr(v, '=');
      pcv_xray_filter* f = filters ? &filters[num_filters] : NULL;
      if (!f || !filter_names || !eq || sscanf(eq + 1, "%lf,%lf", &f->lo, &f->hi) != 2) return usage();
      char* name = (char*)calloc((size_t)(eq - v) + 1, 1);
      if (!name) return usage();
      memcpy(name, v, (size_t)(eq - v));
      filter_names[num_filters] = name;
      f->attribute = name;
      ++num_filters;
    } else if (!strcmp(a, "--root-node-id")) {
      root = v;
    } else if (!strcmp(a, "--inpaint-distance-px")) {
      inpaint = strtol(v, NULL, 10);
      if (inpaint < 0 || inpaint > 255) return usage();
    } else if (!strcmp(a, "--png")) {
      if (!strcmp(v, "stored")) png = PCV_XRAY_PNG_STORED;
      else if (!strcmp(v, "deflate")) png = PCV_XRAY_PNG_DEFLATE;
      else return usage();
    } else {
      return usage();
    }
  }
  if (!inputs || num_inputs == 0 || !output || !(p.pixel_size_m > 0.0)) return usage();
  /* quadtree NodeId from its Display form: "r" and one base-4 digit per level */
  if (root[0] != 'r') return usage();
  for (const char* c = root + 1; *c; ++c) {
    if (*c < '0' || *c > '3') return usage();
    p.root_index = (p.root_index << 2) | (uint64_t)(*c - '0');
    ++p.root_level;
  }
  pcv_ctx* ctx = NULL;
  pcv_octree** trees = (pcv_octree**)calloc(num_inputs, sizeof(pcv_octree*));
  pcv_s2_cloud** clouds = (pcv_s2_cloud**)calloc(num_inputs, sizeof(pcv_s2_cloud*));
  int kind = PCV_CLOUD_OCTREE;
  pcv_xray* x = NULL;
  const uint32_t background = p.background;
  if (inpaint >= 0) p.background = PCV_XRAY_BG_TRANSPARENT; /* the holes must survive until they are filled */
  int rc = trees && clouds ? pcv_cloud_kind(inputs[0], &kind) : PCV_E_OOM;
  if (rc != PCV_OK) {
    fprintf(stderr, "build_xray_quadtree: %s (%d)\n", trees && clouds ? pcv_host_last_error() : "out of memory", rc);
    free(trees);
    free(clouds);
    free(inputs);
    return 1;
  }
  if (kind != PCV_CLOUD_S2 && num_filters) { /* an octree takes one interval, on intensity (the library checks the name) */
    p.interval_attribute = filters[num_filters - 1].attribute;
    p.interval[0] = filters[num_filters - 1].lo;
    p.interval[1] = filters[num_filters - 1].hi;
  }
  rc = pcv_ctx_create(0, NULL, &ctx);
  for (uint32_t t = 0; t < num_inputs && rc == PCV_OK; ++t)
    rc = kind == PCV_CLOUD_S2 ? pcv_s2_open_dir(ctx, inputs[t], &clouds[t]) : pcv_octree_open_dir(ctx, inputs[t], &trees[t]);
  if (rc == PCV_OK)
    rc = kind == PCV_CLOUD_S2 ? pcv_xray_run_s2_ex(ctx, clouds, num_inputs, &p, &col, filters, num_filters, &x)
                              : pcv_xray_run_ex(ctx, trees, num_inputs, &p, &col, &x);
  if (rc == PCV_OK && inpaint >= 0) { /* the result carries its own parent levels */
    pcv_xray* filled = NULL;
    rc = pcv_xray_inpaint(ctx, x, NULL, 0, (uint32_t)inpaint, background, &filled);
    if (rc == PCV_OK) {
      pcv_xray_free(x);
      x = filled;
    }
  } else if (rc == PCV_OK) {
    rc = pcv_xray_build_parents(x);
  }
  if (rc == PCV_OK) rc = pcv_xray_write_dir_ex(x, output, png);
  if (rc == PCV_OK) {
    uint64_t nodes = 0, created = 0;
    uint32_t deepest = 0;
    pcv_xray_nodes(x, &nodes, 0, NULL, NULL);
    pcv_xray_info(x, &deepest, NULL, NULL, &created);
    printf("%llu nodes (%llu leaf tiles at level %u) written to %s\n", (unsigned long long)nodes, (unsigned long long)created, deepest,
           output);
  } else {
    fprintf(stderr, "build_xray_quadtree: %s (%d)\n", ctx ? pcv_last_error(ctx) : "no context", rc);
  }
  pcv_xray_free(x);
  for (uint32_t t = 0; t < num_inputs; ++t) {
    if (trees[t]) pcv_octree_free(trees[t]);
    if (clouds[t]) pcv_s2_free(clouds[t]);
  }
  free(trees);
  free(clouds);
  free(inputs);
  for (uint32_t k = 0; k < num_filters; ++k) free(filter_names[k]);
  free(filter_names);
  free(filters);
  if (ctx) pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
