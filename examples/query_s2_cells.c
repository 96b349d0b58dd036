/* query_s2_cells.c — point queries over an S2 cell cloud directory, in plain C11 on top of the C ABI: what the reference's
 * S2Cells::from_data_provider, nodes_in_location and stream_points_for_query_in_node (src/s2_cells/mod.rs) do for one query,
 * here for many locations in one call. The call sequence of a non-Python host:
 *   pcv_s2_open_dir -> pcv_shapes_create (N x N AABB tiles over the bounding box) [+ one cell union] ->
 *   pcv_s2_cells_in_location (the cells of every location) -> pcv_s2_query_run_ex / _segments (their points, kept on the device)
 * --filter NAME:LO:HI (iterator.rs:66-119) keeps, in every location, the points whose scalar attribute NAME — `intensity` or one
 * of the extras that pcv_s2_attributes lists — lies in [LO, HI]; it may be given several times, once per attribute.
 *
 *   query_s2_cells <directory> [--tiles 4] [--cell <token>] [--filter NAME:LO:HI]...
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static int usage(void) {
  fprintf(stderr, "usage: query_s2_cells <directory> [--tiles 4] [--cell <token>] [--filter NAME:LO:HI]...\n");
  return 2;
}

/* CellID::from_token: hex digits, padded with zeros to 16 */
static uint64_t cell_of_token(const char* token) {
  const size_t len = strlen(token);
  if (len == 0 || len > 16) return 0;
  uint64_t id = 0;
  for (size_t k = 0; k < 16; ++k) {
    unsigned digit = 0;
    if (k < len) {
      const char ch = token[k];
      if (ch >= '0' && ch <= '9') digit = (unsigned)(ch - '0');
      else if (ch >= 'a' && ch <= 'f') digit = (unsigned)(ch - 'a' + 10);
      else return 0;
    }
    id = (id << 4) | digit;
  }
  return id;
}

#define MAX_FILTERS 17 /* intensity and PCV_S2_MAX_EXTRAS extras */

/* NAME:LO:HI, split in place at its last two colons */
static int parse_filter(char* arg, const char** name, double* lo, double* hi) {
  char* c2 = strrchr(arg, ':');
  if (!c2) return 0;
  *c2 = '\0';
  char* c1 = strrchr(arg, ':');
  if (!c1 || c1 == arg) return 0;
  *c1 = '\0';
  char *end1, *end2;
  *lo = strtod(c1 + 1, &end1);
  *hi = strtod(c2 + 1, &end2);
  *name = arg;
  return end1 != c1 + 1 && *end1 == '\0' && end2 != c2 + 1 && *end2 == '\0';
}

int main(int argc, char** argv) {
  const char* dir = NULL;
  const char* token = NULL;
  long tiles = 4;
  const char* filter_name[MAX_FILTERS];
  double filter_lo[MAX_FILTERS], filter_hi[MAX_FILTERS];
  uint32_t num_names = 0;
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--tiles") == 0 && i + 1 < argc) tiles = atol(argv[++i]);
    else if (strcmp(argv[i], "--filter") == 0 && i + 1 < argc && num_names < MAX_FILTERS) {
      if (!parse_filter(argv[++i], &filter_name[num_names], &filter_lo[num_names], &filter_hi[num_names])) return usage();
      ++num_names;
    }
    else if (strcmp(argv[i], "--cell") == 0 && i + 1 < argc) token = argv[++i];
    else if (argv[i][0] != '-' && !dir) dir = argv[i];
    else return usage();
  }
  if (!dir || tiles < 0 || tiles > 1000) return usage();
  uint64_t union_cell = token ? cell_of_token(token) : 0;
  if (token && !union_cell) {
    fprintf(stderr, "%s is no cell token\n", token);
    return 2;
  }

  pcv_ctx* ctx = NULL;
  int rc;
  if ((rc = pcv_ctx_create(0, NULL, &ctx)) != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    return 1;
  }
  pcv_s2_cloud* cloud = NULL;
  if ((rc = pcv_s2_open_dir(ctx, dir, &cloud)) != PCV_OK) {
    fprintf(stderr, "cannot open %s (%d): %s\n", dir, rc, pcv_last_error(ctx));
    pcv_ctx_destroy(ctx);
    return 1;
  }
  uint64_t num_cells = 0, num_points = 0;
  double lo[3], hi[3];
  pcv_s2_info(cloud, &num_cells, &num_points, lo, hi, NULL, NULL);
  printf("%s: %llu cells, %llu points\n", dir, (unsigned long long)num_cells, (unsigned long long)num_points);
  uint32_t num_extras = 0;
  const char* extra_names[PCV_S2_MAX_EXTRAS];
  int32_t extra_types[PCV_S2_MAX_EXTRAS];
  pcv_s2_attributes(cloud, &num_extras, extra_names, extra_types);
  for (uint32_t k = 0; k < num_extras; ++k) printf("  attribute %s: data type %d\n", extra_names[k], (int)extra_types[k]);

  const uint32_t num_shapes = (uint32_t)(tiles * tiles), num_unions = token ? 1u : 0u, locations = num_shapes + num_unions;
  pcv_shape* specs = (pcv_shape*)calloc(num_shapes ? num_shapes : 1, sizeof(pcv_shape));
  uint32_t* counts = (uint32_t*)calloc(locations ? locations : 1, sizeof(uint32_t));
  uint64_t* first = (uint64_t*)calloc((size_t)locations + 1, sizeof(uint64_t));
  pcv_shapes* shapes = NULL;
  pcv_s2_query* query = NULL;
  uint64_t* offset = NULL;
  /* every filter on every location */
  const uint32_t num_filters = num_names * locations;
  pcv_s2_filter* filters = (pcv_s2_filter*)calloc(num_filters ? num_filters : 1, sizeof(pcv_s2_filter));
  if (!specs || !counts || !first || !filters) rc = PCV_E_OOM;
  for (uint32_t l = 0; rc == PCV_OK && l < locations; ++l)
    for (uint32_t k = 0; k < num_names; ++k) {
      pcv_s2_filter* f = &filters[l * num_names + k];
      f->location = l;
      f->attribute = filter_name[k];
      f->lo = filter_lo[k];
      f->hi = filter_hi[k];
    }
  for (long a = 0; rc == PCV_OK && a < tiles; ++a)
    for (long b = 0; b < tiles; ++b) {
      pcv_shape* s = &specs[a * tiles + b];
      s->kind = PCV_SHAPE_AABB;
      s->params[0] = lo[0] + (hi[0] - lo[0]) * (double)a / (double)tiles;
      s->params[1] = lo[1] + (hi[1] - lo[1]) * (double)b / (double)tiles;
      s->params[2] = lo[2];
      s->params[3] = lo[0] + (hi[0] - lo[0]) * (double)(a + 1) / (double)tiles;
      s->params[4] = lo[1] + (hi[1] - lo[1]) * (double)(b + 1) / (double)tiles;
      s->params[5] = hi[2];
    }
  const uint32_t union_first[2] = {0, 1};
  if (rc == PCV_OK && num_shapes) rc = pcv_shapes_create(ctx, specs, num_shapes, &shapes);
  /* capacity 0: the counts alone */
  if (rc == PCV_OK) rc = pcv_s2_cells_in_location(cloud, shapes, num_unions, union_first, &union_cell, 0, counts, NULL);
  if (rc == PCV_OK) rc = pcv_s2_query_run_ex(cloud, shapes, num_unions, union_first, &union_cell, filters, num_filters, &query);
  uint64_t num_segments = 0, kept = 0;
  if (rc == PCV_OK) rc = pcv_s2_query_sizes(query, &num_segments, &kept);
  if (rc == PCV_OK && !(offset = (uint64_t*)calloc((size_t)num_segments + 1, sizeof(uint64_t)))) rc = PCV_E_OOM;
  if (rc == PCV_OK) rc = pcv_s2_query_segments(query, first, NULL, offset);
  if (rc != PCV_OK) {
    fprintf(stderr, "query failed (%d): %s\n", rc, pcv_last_error(ctx));
  } else {
    for (uint32_t l = 0; l < locations; ++l) {
      if (l < num_shapes) printf("tile %u", l);
      else printf("cell %s", token);
      printf(": %u cells, %llu points\n", counts[l], (unsigned long long)(offset[first[l + 1]] - offset[first[l]]));
    }
    printf("%u locations: %llu segments, %llu points\n", locations, (unsigned long long)num_segments, (unsigned long long)kept);
  }
  pcv_s2_query_free(query);
  if (shapes) pcv_shapes_free(shapes);
  pcv_s2_free(cloud);
  pcv_ctx_destroy(ctx);
  free(offset);
  free(filters);
  free(first);
  free(counts);
  free(specs);
  return rc == PCV_OK ? 0 : 1;
}
