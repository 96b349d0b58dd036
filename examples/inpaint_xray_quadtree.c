/* inpaint_xray_quadtree.c — xray's inpaint_xray_quadtree (xray/src/bin/inpaint_xray_quadtree.rs) over the C ABI in plain
 * C11: the (possibly partial) quadtree with root --root-node-id of the input directory is opened with the quadtrees whose
 * roots are its Left, Top, Right and Bottom neighbours (pcv_xray_open_dir), the holes of its leaf tiles are filled on the
 * device with their adjacent leaves as context (pcv_xray_inpaint), and the inpainted quadtree, its parent levels rebuilt,
 * is written (pcv_xray_write_dir_ex). The output directory may be the input. Everything but the fill is the reference's,
 * byte for byte; the fill is a distance-weighted mean, not the reference's texture synthesis.
 *
 *   inpaint_xray_quadtree <input dir> --output-directory <dir> --inpaint-distance-px <0..254>
 *                         [--tile-background-color white|transparent] [--root-node-id <r...>] [--png stored|deflate]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static int usage(void) {
  fprintf(stderr, "usage: inpaint_xray_quadtree <input dir> --output-directory <dir> --inpaint-distance-px <0..254>\n"
                  "       [--tile-background-color white|transparent] [--root-node-id <r...>] [--png stored|deflate]\n");
  return 2;
}

/* the root of an opened quadtree: its node of minimum level (Meta::get_root_node) */
static int root_of(const pcv_xray* x, uint32_t* level, uint64_t* index) {
  uint64_t n = 0;
  pcv_xray_nodes(x, &n, 0, NULL, NULL);
  if (n == 0) return 0;
  uint32_t* levels = (uint32_t*)calloc(n, sizeof(uint32_t));
  uint64_t* indices = (uint64_t*)calloc(n, sizeof(uint64_t));
  pcv_xray_nodes(x, &n, n, levels, indices);
  uint64_t at = 0;
  for (uint64_t i = 1; i < n; ++i)
    if (levels[i] < levels[at]) at = i;
  *level = levels[at];
  *index = indices[at];
  free(levels);
  free(indices);
  return 1;
}

/* SpatialNodeId::from(NodeId) and back (quadtree/src/lib.rs:314-349) */
static void spatial(uint32_t level, uint64_t index, int64_t* x, int64_t* y) {
  *x = *y = 0;
  for (uint32_t b = 0; b < level; ++b) {
    *y |= (int64_t)((index >> (2 * b)) & 1u) << b;
    *x |= (int64_t)((index >> (2 * b + 1)) & 1u) << b;
  }
}
static uint64_t node_index(uint32_t level, int64_t x, int64_t y) {
  uint64_t index = 0;
  for (uint32_t b = 0; b < level; ++b) index |= (((uint64_t)y >> b) & 1u) << (2 * b) | (((uint64_t)x >> b) & 1u) << (2 * b + 1);
  return index;
}

int main(int argc, char** argv) {
  const char *input = NULL, *output = NULL, *root = "r";
  uint32_t background = PCV_XRAY_BG_WHITE;
  long distance = -1;
  int png = PCV_XRAY_PNG_STORED;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (a[0] != '-') {
      if (input) return usage();
      input = a;
      continue;
    }
    if (i + 1 >= argc) return usage();
    const char* v = argv[++i];
    if (!strcmp(a, "--output-directory")) {
      output = v;
    } else if (!strcmp(a, "--inpaint-distance-px")) {
      distance = strtol(v, NULL, 10);
      if (distance < 0 || distance > 255) return usage();
    } else if (!strcmp(a, "--tile-background-color")) {
      if (!strcmp(v, "white")) background = PCV_XRAY_BG_WHITE;
      else if (!strcmp(v, "transparent")) background = PCV_XRAY_BG_TRANSPARENT;
      else return usage();
    } else if (!strcmp(a, "--root-node-id")) {
      root = v;
    } else if (!strcmp(a, "--png")) {
      if (!strcmp(v, "stored")) png = PCV_XRAY_PNG_STORED;
      else if (!strcmp(v, "deflate")) png = PCV_XRAY_PNG_DEFLATE;
      else return usage();
    } else {
      return usage();
    }
  }
  if (!input || !output || distance < 0 || root[0] != 'r') return usage();
  uint32_t root_level = 0;
  uint64_t root_index = 0;
  for (const char* c = root + 1; *c; ++c) {
    if (*c < '0' || *c > '3') return usage();
    root_index = (root_index << 2) | (uint64_t)(*c - '0');
    ++root_level;
  }
  pcv_ctx* ctx = NULL;
  if (pcv_ctx_create(0, NULL, &ctx) != PCV_OK) {
    fprintf(stderr, "no device context\n");
    return 1;
  }
  uint32_t total = 0;
  int rc = pcv_xray_open_dir(ctx, input, 0, NULL, &total);
  pcv_xray** parts = (pcv_xray**)calloc((size_t)total + 1, sizeof(pcv_xray*));
  if (rc == PCV_OK) rc = pcv_xray_open_dir(ctx, input, total, parts, &total);
  /* the quadtree itself and the ones whose roots are root.neighbor(Left / Top / Right / Bottom), bin :53-59 */
  static const int dx[4] = {-1, 0, 1, 0}, dy[4] = {0, 1, 0, -1};
  pcv_xray* x = NULL;
  pcv_xray* neighbours[4];
  uint32_t num_neighbours = 0;
  int64_t rx, ry;
  spatial(root_level, root_index, &rx, &ry);
  for (uint32_t k = 0; rc == PCV_OK && k < total; ++k) {
    uint32_t level;
    uint64_t index;
    if (!root_of(parts[k], &level, &index) || level != root_level) continue;
    if (index == root_index) x = parts[k];
    for (int t = 0; t < 4; ++t) {
      const int64_t nx = rx + dx[t], ny = ry + dy[t], dim = (int64_t)1 << root_level;
      if (nx >= 0 && nx < dim && ny >= 0 && ny < dim && node_index(root_level, nx, ny) == index && num_neighbours < 4)
        neighbours[num_neighbours++] = parts[k];
    }
  }
  pcv_xray* out = NULL;
  if (rc == PCV_OK && !x) {
    fprintf(stderr, "inpaint_xray_quadtree: no quadtree with root %s in %s\n", root, input);
    rc = PCV_E_NOT_FOUND;
  } else if (rc == PCV_OK) {
    uint64_t adjacent = 0;
    char err[256];
    rc = pcv_xray_inpaint_plan(x, neighbours, num_neighbours, 0, NULL, &adjacent, err, sizeof(err));
    if (rc != PCV_OK) fprintf(stderr, "inpaint_xray_quadtree: %s\n", err);
    else if (root_level != 0 && adjacent == 0)
      fprintf(stderr, "No adjacent leaf nodes found in neighboring quadtrees. Did you forget to copy them into \"%s\"?\n", input);
    if (rc == PCV_OK) {
      rc = pcv_xray_inpaint(ctx, x, neighbours, num_neighbours, (uint32_t)distance, background, &out);
      if (rc == PCV_OK) rc = pcv_xray_write_dir_ex(out, output, png);
      if (rc != PCV_OK) fprintf(stderr, "inpaint_xray_quadtree: %s\n", pcv_last_error(ctx));
    }
  } else {
    fprintf(stderr, "inpaint_xray_quadtree: %s\n", pcv_last_error(ctx));
  }
  if (rc == PCV_OK) {
    uint64_t nodes = 0, leaves = 0, target = 0, filled = 0;
    pcv_xray_nodes(out, &nodes, 0, NULL, NULL);
    pcv_xray_info(out, NULL, NULL, &leaves, NULL);
    uint64_t* t = (uint64_t*)calloc(leaves + 1, sizeof(uint64_t));
    uint64_t* f = (uint64_t*)calloc(leaves + 1, sizeof(uint64_t));
    pcv_xray_inpaint_info(out, t, f, NULL);
    for (uint64_t i = 0; i < leaves; ++i) target += t[i], filled += f[i];
    free(t);
    free(f);
    printf("inpainted %s of %s with %u neighbour quadtrees: %llu leaves, %llu target pixels, %llu filled; %llu nodes written to %s\n", root,
           input, num_neighbours, (unsigned long long)leaves, (unsigned long long)target, (unsigned long long)filled,
           (unsigned long long)nodes, output);
  }
  pcv_xray_free(out);
  for (uint32_t k = 0; k < total; ++k) pcv_xray_free(parts[k]);
  free(parts);
  pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
