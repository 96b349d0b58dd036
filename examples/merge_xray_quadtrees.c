/* merge_xray_quadtrees.c — xray's merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs) over the C ABI in plain
 * C11: every partial quadtree (meta*.pb) of the input directories is opened (pcv_xray_open_dir), checked and merged with
 * the levels above the parts' roots built on the device (pcv_xray_merge), and the quadtree with root r is written
 * (pcv_xray_write_dir_ex): the parts' PNGs copied, the new levels encoded (--png deflate: compressed on the device),
 * meta.pb with the union node list. The output directory may be one of the inputs.
 *
 *   merge_xray_quadtrees --output-directory <dir> [--tile-background-color white|transparent] [--png stored|deflate]
 *                        <input dir>...
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "pcv_layout_check.h"

static int usage(void) {
  fprintf(stderr, "usage: merge_xray_quadtrees --output-directory <dir> [--tile-background-color white|transparent] [--png stored|deflate] <input dir>...\n");
  return 2;
}

int main(int argc, char** argv) {
  const char** inputs = (const char**)calloc((size_t)argc + 1, sizeof(const char*));
  uint32_t num_inputs = 0, background = PCV_XRAY_BG_WHITE;
  const char* output = NULL;
  int png = PCV_XRAY_PNG_STORED;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (a[0] != '-') {
      inputs[num_inputs++] = a;
      continue;
    }
    if (i + 1 >= argc) return usage();
    const char* v = argv[++i];
    if (!strcmp(a, "--output-directory")) {
      output = v;
    } else if (!strcmp(a, "--tile-background-color")) {
      if (!strcmp(v, "white")) background = PCV_XRAY_BG_WHITE;
      else if (!strcmp(v, "transparent")) background = PCV_XRAY_BG_TRANSPARENT;
      else return usage();
    } else if (!strcmp(a, "--png")) {
      if (!strcmp(v, "stored")) png = PCV_XRAY_PNG_STORED;
      else if (!strcmp(v, "deflate")) png = PCV_XRAY_PNG_DEFLATE;
      else return usage();
    } else {
      return usage();
    }
  }
  if (!output || num_inputs == 0) return usage();
  for (uint32_t k = 0; k < num_inputs; ++k) { /* validate_input_directory :113-127 */
    struct stat st;
    if (stat(inputs[k], &st) != 0) {
      fprintf(stderr, "Input directory \"%s\" doesn't exist.\n", inputs[k]);
      return 1;
    }
    if (!S_ISDIR(st.st_mode)) {
      fprintf(stderr, "\"%s\" is not a directory.\n", inputs[k]);
      return 1;
    }
  }
  pcv_ctx* ctx = NULL;
  if (pcv_ctx_create(0, NULL, &ctx) != PCV_OK) {
    fprintf(stderr, "no device context\n");
    return 1;
  }
  int rc = PCV_OK;
  uint32_t total = 0;
  uint32_t* counts = (uint32_t*)calloc(num_inputs, sizeof(uint32_t));
  for (uint32_t k = 0; rc == PCV_OK && k < num_inputs; ++k) {
    rc = pcv_xray_open_dir(ctx, inputs[k], 0, NULL, &counts[k]);
    total += counts[k];
  }
  pcv_xray** parts = (pcv_xray**)calloc((size_t)total + 1, sizeof(pcv_xray*));
  uint32_t at = 0;
  for (uint32_t k = 0; rc == PCV_OK && k < num_inputs; ++k) {
    rc = pcv_xray_open_dir(ctx, inputs[k], counts[k], parts + at, &counts[k]);
    at += counts[k];
  }
  pcv_xray* merged = NULL;
  if (rc == PCV_OK) rc = pcv_xray_merge(ctx, parts, total, background, &merged);
  if (rc == PCV_OK) rc = pcv_xray_write_dir_ex(merged, output, png);
  if (rc == PCV_OK) {
    uint64_t nodes = 0;
    uint32_t deepest = 0;
    double rect[3];
    pcv_xray_nodes(merged, &nodes, 0, NULL, NULL);
    pcv_xray_info(merged, &deepest, rect, NULL, NULL);
    printf("merged %u partial quadtrees into %s: %llu nodes, deepest level %u, rect min (%g, %g) edge %g\n", total, output,
           (unsigned long long)nodes, deepest, rect[0], rect[1], rect[2]);
  } else {
    fprintf(stderr, "merge_xray_quadtrees: %s\n", pcv_last_error(ctx));
  }
  pcv_xray_free(merged);
  for (uint32_t k = 0; k < total; ++k) pcv_xray_free(parts[k]);
  pcv_ctx_destroy(ctx);
  free(parts);
  free(counts);
  free(inputs);
  return rc == PCV_OK ? 0 : 1;
}
