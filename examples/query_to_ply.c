/* query_to_ply.c — "the points under these map tiles, as a PLY", in plain C11 on top of the C ABI: what the reference does with
 * a PointQuery, stream_points_for_query and a PlyNodeWriter (src/read_write/ply.rs:559-732), over an octree directory or an S2
 * cell cloud directory (pcv_cloud_kind decides). The call sequence of a non-Python host:
 *   pcv_cloud_kind -> pcv_octree_open_dir | pcv_s2_open_dir -> pcv_shapes_create[_ex | _ex2] -> pcv_query_batch_run |
 *   pcv_s2_query_run_ex -> pcv_query_batch_write_ply | pcv_s2_query_write_ply
 * The rows are packed on the device and reach the file in pieces: no point array is held on the host.
 *
 *   query_to_ply <cloud dir> (--aabb x0,y0,z0,x1,y1,z1 | --cells tok,.. | --map-tiles z | --all) [--filter NAME:LO:HI]
 *                [--attributes a,b] --output out.ply [--append] [--per-location out_%u.ply]
 *   query_to_ply <cloud dir> --polygon FILE [--polygon-frame xy|web-mercator] [--z LO,HI] [the options above]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: query_to_ply <cloud dir> (--aabb x0,y0,z0,x1,y1,z1 | --cells tok,.. | --map-tiles z | --all) [--filter NAME:LO:HI]\n"
    "                    [--attributes a,b] --output out.ply [--append] [--per-location out_%u.ply]\n"
    "       query_to_ply <cloud dir> --polygon FILE [--polygon-frame xy|web-mercator] [--z LO,HI] [the options above]\n"
    "  <cloud dir>       an octree directory or an S2 cell cloud directory (meta.pb decides)\n"
    "  --aabb            one location: an axis-aligned box in the cloud's coordinates\n"
    "  --cells           one location: the union of these S2 cells (tokens, ascending by id), over ECEF points\n"
    "  --map-tiles z     one location per web-mercator tile of zoom z (0 ..= 23) that the bounding box touches, over ECEF points\n"
    "  --polygon FILE    one location: the polygon (even-odd) whose rings FILE holds, one `x y` pair per line, a blank line\n"
    "                    between rings; the per-node counts are printed\n"
    "  --polygon-frame   xy (default): the pairs are in the cloud's own x and y; web-mercator: they are `lat lng` in degrees,\n"
    "                    over ECEF points\n"
    "  --z LO,HI         the polygon's closed height range in the xy frame (default: unbounded)\n"
    "  --all             one location: every point\n"
    "  --filter          keep the points whose scalar attribute NAME lies in [LO, HI]; an octree knows `intensity` only\n"
    "  --attributes      the columns of a row behind x y z (default: every attribute of the cloud; an empty list: positions only)\n"
    "  --output          the file that takes every location's points, one location after the other\n"
    "  --append          add to the file (its columns must be the same) where --output alone writes it anew\n"
    "  --per-location    also one file per location that has points; %u is the location's index\n";

static int usage(void) {
  fputs(kUsage, stderr);
  return 2;
}

/* CellID::from_token: hex digits, padded with zeros to 16 */
static uint64_t cell_of_token(const char* token, size_t len) {
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

/* a,b,c split in place; returns the number of fields, -1 when there are more than cap */
static int split_commas(char* arg, const char** fields, int cap) {
  int n = 0;
  if (!*arg) return 0;
  for (char* at = arg;;) {
    if (n == cap) return -1;
    fields[n++] = at;
    char* comma = strchr(at, ',');
    if (!comma) return n;
    *comma = '\0';
    at = comma + 1;
  }
}

#define MAX_FILTERS 17 /* intensity and PCV_S2_MAX_EXTRAS extras */
#define MAX_ATTRS 18   /* color, intensity and the extras */
#define MAX_CELLS 4096
#define MAX_TILES 4096

#define MAX_RINGS 4096
#define MAX_VERTICES 65535

enum { LOC_NONE, LOC_AABB, LOC_CELLS, LOC_TILES, LOC_ALL, LOC_POLYGON };

/* one `x y` pair per line, a blank line between rings: ring_first (num_rings + 1 offsets) and the pairs */
static int read_rings(const char* path, uint32_t* ring_first, uint32_t* num_rings, double* vertices, uint32_t* num_vertices) {
  FILE* f = fopen(path, "r");
  if (!f) return 0;
  char line[256];
  uint32_t nr = 0, nv = 0;
  int open = 0, ok = 1;
  ring_first[0] = 0;
  while (ok && fgets(line, sizeof(line), f)) {
    double a, b;
    if (sscanf(line, "%lf %lf", &a, &b) == 2) {
      if (nv == MAX_VERTICES) ok = 0;
      else vertices[2 * nv] = a, vertices[2 * nv + 1] = b, ++nv, open = 1;
    } else if (line[strspn(line, " \t\r\n")] == '\0') { /* a blank line closes the ring */
      if (open && nr < MAX_RINGS) ring_first[++nr] = nv;
      else if (open) ok = 0;
      open = 0;
    } else {
      ok = 0;
    }
  }
  if (ok && open && nr < MAX_RINGS) ring_first[++nr] = nv;
  else if (open) ok = 0;
  fclose(f);
  *num_rings = nr, *num_vertices = nv;
  return ok;
}

int main(int argc, char** argv) {
  const char *dir = NULL, *output = NULL, *pattern = NULL, *polygon_file = NULL;
  int web_mercator = 0;
  double z_range[2] = {-1.0 / 0.0, 1.0 / 0.0};
  int location = LOC_NONE, append = 0, have_attrs = 0, num_attrs = 0, num_filters = 0;
  double box[6] = {0};
  long zoom = -1;
  const char* attrs[MAX_ATTRS];
  const char* filter_name[MAX_FILTERS];
  double filter_lo[MAX_FILTERS], filter_hi[MAX_FILTERS];
  static uint64_t cells[MAX_CELLS];
  uint32_t num_cells = 0;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    if (strcmp(a, "--help") == 0 || strcmp(a, "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    } else if (strcmp(a, "--aabb") == 0 && more && location == LOC_NONE) {
      const char* f[6];
      if (split_commas(argv[++i], f, 6) != 6) return usage();
      for (int k = 0; k < 6; ++k) {
        char* end;
        box[k] = strtod(f[k], &end);
        if (end == f[k] || *end) return usage();
      }
      location = LOC_AABB;
    } else if (strcmp(a, "--cells") == 0 && more && location == LOC_NONE) {
      static const char* f[MAX_CELLS];
      const int n = split_commas(argv[++i], f, MAX_CELLS);
      if (n <= 0) return usage();
      for (int k = 0; k < n; ++k)
        if (!(cells[k] = cell_of_token(f[k], strlen(f[k])))) {
          fprintf(stderr, "%s is no cell token\n", f[k]);
          return 2;
        }
      num_cells = (uint32_t)n;
      location = LOC_CELLS;
    } else if (strcmp(a, "--map-tiles") == 0 && more && location == LOC_NONE) {
      char* end;
      zoom = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || zoom < 0 || zoom > 23) return usage();
      location = LOC_TILES;
    } else if (strcmp(a, "--polygon") == 0 && more && location == LOC_NONE) {
      polygon_file = argv[++i];
      location = LOC_POLYGON;
    } else if (strcmp(a, "--polygon-frame") == 0 && more) {
      ++i;
      if (strcmp(argv[i], "xy") != 0 && strcmp(argv[i], "web-mercator") != 0) return usage();
      web_mercator = strcmp(argv[i], "web-mercator") == 0;
    } else if (strcmp(a, "--z") == 0 && more) {
      const char* f[2];
      if (split_commas(argv[++i], f, 2) != 2) return usage();
      for (int k = 0; k < 2; ++k) {
        char* end;
        z_range[k] = strtod(f[k], &end);
        if (end == f[k] || *end) return usage();
      }
    } else if (strcmp(a, "--all") == 0 && location == LOC_NONE) {
      location = LOC_ALL;
    } else if (strcmp(a, "--filter") == 0 && more && num_filters < MAX_FILTERS) {
      if (!parse_filter(argv[++i], &filter_name[num_filters], &filter_lo[num_filters], &filter_hi[num_filters])) return usage();
      ++num_filters;
    } else if (strcmp(a, "--attributes") == 0 && more && !have_attrs) {
      if ((num_attrs = split_commas(argv[++i], attrs, MAX_ATTRS)) < 0) return usage();
      have_attrs = 1;
    } else if (strcmp(a, "--output") == 0 && more && !output) {
      output = argv[++i];
    } else if (strcmp(a, "--per-location") == 0 && more && !pattern) {
      pattern = argv[++i];
      const char* mark = strstr(pattern, "%u");
      if (!mark || strchr(mark + 1, '%') || strchr(pattern, '%') != mark) return usage(); /* exactly one %u, no other % */
    } else if (strcmp(a, "--append") == 0) {
      append = 1;
    } else if (a[0] != '-' && !dir) {
      dir = a;
    } else {
      return usage();
    }
  }
  if (!dir || !output || location == LOC_NONE) return usage();

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
  pcv_shape* specs = NULL;
  double *intervals = NULL, lo[3], hi[3];
  pcv_s2_filter* filters = NULL;
  uint64_t *first = NULL, *offset = NULL;
  static uint32_t ring_first[MAX_RINGS + 1];
  static double vertices[2 * MAX_VERTICES];
  uint32_t num_rings = 0, num_vertices = 0;
  const char* what = "open";
  rc = kind == PCV_CLOUD_S2 ? pcv_s2_open_dir(ctx, dir, &cloud) : pcv_octree_open_dir(ctx, dir, &tree);
  if (rc != PCV_OK) goto done;
  if (cloud) pcv_s2_info(cloud, NULL, NULL, lo, hi, NULL, NULL);
  else pcv_octree_meta(tree, NULL, lo, hi, NULL);

  /* ---- the locations ---- */
  what = "locations";
  uint32_t num_shapes = 0, num_unions = 0;
  const uint32_t union_first[2] = {0, num_cells};
  if (location == LOC_TILES) {
    /* the tiles of zoom z that the bounding box's corners span */
    double cx[8], cy[8], cz[8], u[8], v[8];
    for (int k = 0; k < 8; ++k) cx[k] = k & 1 ? hi[0] : lo[0], cy[k] = k & 2 ? hi[1] : lo[1], cz[k] = k & 4 ? hi[2] : lo[2];
    if ((rc = pcv_wmr_project(8, cx, cy, cz, u, v)) != PCV_OK) goto done;
    const double per_axis = (double)(1ul << zoom);
    double t0[2] = {per_axis, per_axis}, t1[2] = {0, 0};
    for (int k = 0; k < 8; ++k) {
      const double tx = (double)(long)(u[k] * per_axis), ty = (double)(long)(v[k] * per_axis);
      t0[0] = tx < t0[0] ? tx : t0[0], t0[1] = ty < t0[1] ? ty : t0[1];
      t1[0] = tx > t1[0] ? tx : t1[0], t1[1] = ty > t1[1] ? ty : t1[1];
    }
    const double nx = t1[0] - t0[0] + 1, ny = t1[1] - t0[1] + 1;
    if (!(nx >= 1 && ny >= 1 && nx * ny <= MAX_TILES)) {
      fprintf(stderr, "the bounding box spans %.0f x %.0f tiles at zoom %ld: at most %d, choose a lower zoom\n", nx, ny, zoom, MAX_TILES);
      rc = PCV_E_INVALID;
      goto cleanup;
    }
    num_shapes = (uint32_t)(nx * ny);
    if (!(specs = (pcv_shape*)calloc(num_shapes, sizeof(pcv_shape)))) rc = PCV_E_OOM;
    for (uint32_t k = 0; rc == PCV_OK && k < num_shapes; ++k) {
      const double tx = t0[0] + (double)(k % (uint32_t)nx), ty = t0[1] + (double)(k / (uint32_t)nx);
      const double tile_min[2] = {256.0 * tx, 256.0 * ty}, tile_max[2] = {256.0 * (tx + 1), 256.0 * (ty + 1)};
      specs[k].kind = PCV_SHAPE_WEB_MERCATOR_RECT;
      rc = pcv_wmr_from_zoomed(tile_min, tile_max, (uint32_t)zoom, specs[k].params);
    }
    if (rc != PCV_OK) {
      fprintf(stderr, "no web-mercator tiles for this bounding box (%d): %s\n", rc, pcv_host_last_error());
      goto cleanup;
    }
  } else if (location == LOC_POLYGON) {
    if (!read_rings(polygon_file, ring_first, &num_rings, vertices, &num_vertices)) {
      fprintf(stderr, "%s: one `x y` pair per line, a blank line between rings (at most %d rings, %d vertices)\n", polygon_file, MAX_RINGS,
              MAX_VERTICES);
      rc = PCV_E_INVALID;
      goto cleanup;
    }
    if (web_mercator) { /* `lat lng` in degrees -> normalized web-mercator x y */
      static double lat[MAX_VERTICES], lng[MAX_VERTICES], u[MAX_VERTICES], v[MAX_VERTICES];
      for (uint32_t k = 0; k < num_vertices; ++k) lat[k] = vertices[2 * k] * (3.141592653589793 / 180.0), lng[k] = vertices[2 * k + 1] * (3.141592653589793 / 180.0);
      if ((rc = pcv_wmr_from_lat_lng(num_vertices, lat, lng, u, v)) != PCV_OK) goto done;
      for (uint32_t k = 0; k < num_vertices; ++k) vertices[2 * k] = u[k], vertices[2 * k + 1] = v[k];
    }
    num_shapes = 1;
    if (!(specs = (pcv_shape*)calloc(1, sizeof(pcv_shape)))) rc = PCV_E_OOM;
    if (rc == PCV_OK) {
      specs[0].kind = PCV_SHAPE_POLYGON; /* .reserved = 0: the first (and only) polygon */
      specs[0].params[0] = web_mercator ? -1.0 / 0.0 : z_range[0];
      specs[0].params[1] = web_mercator ? 1.0 / 0.0 : z_range[1];
      specs[0].params[2] = web_mercator ? 1.0 : 0.0;
    }
  } else if (location == LOC_CELLS && cloud) {
    num_unions = 1; /* an S2 cloud takes unions beside the shape table */
  } else {
    num_shapes = 1;
    if (!(specs = (pcv_shape*)calloc(1, sizeof(pcv_shape)))) rc = PCV_E_OOM;
    if (rc == PCV_OK) {
      specs[0].kind = location == LOC_AABB ? PCV_SHAPE_AABB : location == LOC_CELLS ? PCV_SHAPE_S2_CELL_UNION : PCV_SHAPE_ALL;
      memcpy(specs[0].params, box, sizeof(box));
    }
  }
  if (rc != PCV_OK) goto done;
  if (num_shapes) {
    const uint32_t one_polygon[2] = {0, num_rings};
    rc = location == LOC_POLYGON ? pcv_shapes_create_ex2(ctx, specs, num_shapes, 0, NULL, NULL, 1, one_polygon, ring_first, vertices, &shapes)
         : location == LOC_CELLS ? pcv_shapes_create_ex(ctx, specs, num_shapes, 1, union_first, cells, &shapes)
                                 : pcv_shapes_create(ctx, specs, num_shapes, &shapes);
    if (rc != PCV_OK) goto done;
  }
  const uint32_t locations = num_shapes + num_unions;

  /* ---- the query: every filter on every location ---- */
  what = "query";
  uint64_t num_segments = 0, num_points = 0;
  if (cloud) {
    const uint32_t total = (uint32_t)num_filters * locations;
    if (!(filters = (pcv_s2_filter*)calloc(total ? total : 1, sizeof(pcv_s2_filter)))) rc = PCV_E_OOM;
    for (uint32_t l = 0; rc == PCV_OK && l < locations; ++l)
      for (int k = 0; k < num_filters; ++k) {
        pcv_s2_filter* f = &filters[l * (uint32_t)num_filters + (uint32_t)k];
        f->location = l, f->attribute = filter_name[k], f->lo = filter_lo[k], f->hi = filter_hi[k];
      }
    if (rc == PCV_OK) rc = pcv_s2_query_run_ex(cloud, shapes, num_unions, union_first, cells, filters, total, &query);
    if (rc == PCV_OK) rc = pcv_s2_query_sizes(query, &num_segments, &num_points);
  } else {
    if (num_filters > 1 || (num_filters == 1 && strcmp(filter_name[0], "intensity") != 0)) {
      fprintf(stderr, "an octree carries color and intensity: --filter takes `intensity` only, once\n");
      rc = PCV_E_INVALID;
      goto cleanup;
    }
    if (num_filters && !(intervals = (double*)calloc(2 * (size_t)locations, sizeof(double)))) rc = PCV_E_OOM;
    for (uint32_t l = 0; rc == PCV_OK && num_filters && l < locations; ++l) intervals[2 * l] = filter_lo[0], intervals[2 * l + 1] = filter_hi[0];
    if (rc == PCV_OK) rc = pcv_query_batch_run(ctx, shapes, tree, intervals, NULL, &batch);
    if (rc == PCV_OK) rc = pcv_query_batch_sizes(batch, &num_segments, &num_points);
  }
  if (rc != PCV_OK) goto done;

  /* ---- the files ---- */
  what = "write";
  pcv_ply_write_params params;
  memset(&params, 0, sizeof(params));
  params.struct_size = (uint32_t)sizeof(params);
  params.open_mode = append ? PCV_PLY_APPEND : PCV_PLY_TRUNCATE;
  params.attributes = have_attrs ? attrs : NULL;
  params.num_attributes = (uint32_t)num_attrs;
  uint64_t written = 0;
  rc = cloud ? pcv_s2_query_write_ply(query, 0, num_segments, output, &params, &written)
             : pcv_query_batch_write_ply(batch, 0, num_segments, output, &params, &written);
  if (rc != PCV_OK) goto done;
  printf("%s: %u locations, %llu segments, %llu points %s %s\n", dir, locations, (unsigned long long)num_segments, (unsigned long long)written,
         append ? "appended to" : "written to", written ? output : "no file (a PLY without points is not written)");
  if (location == LOC_POLYGON && num_segments) { /* the per-node (per-cell) counts */
    uint32_t* node = (uint32_t*)calloc((size_t)num_segments, sizeof(uint32_t));
    uint64_t* at = (uint64_t*)calloc((size_t)num_segments + 1, sizeof(uint64_t));
    uint64_t shape_first[2];
    if (!node || !at) rc = PCV_E_OOM;
    if (rc == PCV_OK) rc = cloud ? pcv_s2_query_segments(query, shape_first, node, at) : pcv_query_batch_segments(batch, shape_first, node, at);
    for (uint64_t k = 0; rc == PCV_OK && k < num_segments; ++k)
      printf("  %s %u: %llu points\n", cloud ? "cell" : "node", node[k], (unsigned long long)(at[k + 1] - at[k]));
    free(node);
    free(at);
    if (rc != PCV_OK) goto done;
  }
  if (pattern) {
    first = (uint64_t*)calloc((size_t)locations + 1, sizeof(uint64_t));
    offset = (uint64_t*)calloc((size_t)num_segments + 1, sizeof(uint64_t));
    char* path = (char*)malloc(strlen(pattern) + 16);
    if (!first || !offset || !path) rc = PCV_E_OOM;
    if (rc == PCV_OK) rc = cloud ? pcv_s2_query_segments(query, first, NULL, offset) : pcv_query_batch_segments(batch, first, NULL, offset);
    const size_t mark = (size_t)(strstr(pattern, "%u") - pattern);
    for (uint32_t l = 0; rc == PCV_OK && l < locations; ++l) {
      sprintf(path, "%.*s%u%s", (int)mark, pattern, l, pattern + mark + 2);
      rc = cloud ? pcv_s2_query_write_ply(query, first[l], first[l + 1] - first[l], path, &params, &written)
                 : pcv_query_batch_write_ply(batch, first[l], first[l + 1] - first[l], path, &params, &written);
      if (rc == PCV_OK && written) printf("  location %u: %llu points -> %s\n", l, (unsigned long long)written, path);
    }
    free(path);
  }

done:
  if (rc != PCV_OK) fprintf(stderr, "%s failed (%d): %s\n", what, rc, pcv_last_error(ctx));
cleanup:
  pcv_query_batch_free(batch);
  if (query) pcv_s2_query_free(query);
  if (shapes) pcv_shapes_free(shapes);
  if (tree) pcv_octree_free(tree);
  if (cloud) pcv_s2_free(cloud);
  pcv_ctx_destroy(ctx);
  free(offset);
  free(first);
  free(filters);
  free(intervals);
  free(specs);
  return rc == PCV_OK ? 0 : 1;
}
