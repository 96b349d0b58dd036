/* query_to_las.c — "the points inside this parcel, as a LAS file", in plain C11 on top of the C ABI, over an octree
 * directory or an S2 cell cloud directory (pcv_cloud_kind decides). The locations are those of query_to_ply.c. The call sequence
 * of a non-Python host:
 *   pcv_cloud_kind -> pcv_octree_open_dir | pcv_s2_open_dir -> pcv_shapes_create[_ex | _ex2] -> pcv_query_batch_run |
 *   pcv_s2_query_run_ex -> pcv_query_batch_write_las | pcv_s2_query_write_las
 * The records are quantised and packed on the device and reach the file in pieces: no point array is held on the host.
 *
 *   query_to_las <cloud dir> (--aabb x0,y0,z0,x1,y1,z1 | --cells tok,.. | --map-tiles z | --polygon FILE | --all)
 *                [--polygon-frame xy|web-mercator] [--z LO,HI] [--scale S] [--offset x,y,z|auto] [--format F] [--fields a,b]
 *                --output out.las [--append] [--per-location out_%u.las] [--info]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: query_to_las <cloud dir> (--aabb x0,y0,z0,x1,y1,z1 | --cells tok,.. | --map-tiles z | --polygon FILE | --all)\n"
    "                    [--polygon-frame xy|web-mercator] [--z LO,HI] [--scale S] [--offset x,y,z|auto] [--format F] [--fields a,b]\n"
    "                    --output out.las [--append] [--per-location out_%u.las] [--info]\n"
    "  <cloud dir>       an octree directory or an S2 cell cloud directory (meta.pb decides)\n"
    "  --aabb            one location: an axis-aligned box in the cloud's coordinates\n"
    "  --cells           one location: the union of these S2 cells (tokens, ascending by id), over ECEF points\n"
    "  --map-tiles z     one location per web-mercator tile of zoom z (0 ..= 23) that the bounding box touches, over ECEF points\n"
    "  --polygon FILE    one location: the polygon (even-odd) whose rings FILE holds, one `x y` pair per line, a blank line\n"
    "                    between rings; --polygon-frame web-mercator: `lat lng` in degrees; --z: the height range in the xy frame\n"
    "  --all             one location: every point\n"
    "  --scale           the scale factor of X Y Z (default 0.001)\n"
    "  --offset          the offset of X Y Z; auto (default): floor(min) per axis of the points written\n"
    "  --format          the point data record format, 0 - 3 or 6 - 8 (default: chosen from what the cloud carries)\n"
    "  --fields          the fields to fill among color, intensity and the LAS names of the cloud's extras (default: all of them)\n"
    "  --output          the file that takes every location's points, one location after the other\n"
    "  --append          add to the file (same format; its scale and offset are used) where --output alone writes it anew\n"
    "  --per-location    also one file per location that has points; %u is the location's index\n"
    "  --info            print what the library reports about the records: format, offset, bounds, counts\n";

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

static int parse_doubles(char* arg, double* out, int n) {
  const char* f[8];
  if (n > 8 || split_commas(arg, f, n) != n) return 0;
  for (int k = 0; k < n; ++k) {
    char* end;
    out[k] = strtod(f[k], &end);
    if (end == f[k] || *end) return 0;
  }
  return 1;
}

#define MAX_FIELDS 14 /* color, intensity and the twelve LAS extras */
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

static void print_info(const pcv_las_write_info* in) {
  printf("  LAS 1.%u, point data record format %u, %u bytes per record, header %u bytes\n", in->version_minor, in->point_format, in->record_length,
         in->header_size);
  printf("  scale %.17g %.17g %.17g, offset %.17g %.17g %.17g\n", in->scale[0], in->scale[1], in->scale[2], in->offset[0], in->offset[1], in->offset[2]);
  printf("  x %.17g .. %.17g, y %.17g .. %.17g, z %.17g .. %.17g\n", in->bounds[1], in->bounds[0], in->bounds[3], in->bounds[2], in->bounds[5],
         in->bounds[4]);
  printf("  %llu records; by return:", (unsigned long long)in->num_records);
  for (int k = 0; k < 15; ++k) printf(" %llu", (unsigned long long)in->by_return[k]);
  printf("\n  out of range %llu, clamped intensities %llu, masked values %llu, extras not written %u\n", (unsigned long long)in->out_of_range,
         (unsigned long long)in->clamped_intensity, (unsigned long long)in->masked_values, in->skipped_extras);
}

int main(int argc, char** argv) {
  const char *dir = NULL, *output = NULL, *pattern = NULL, *polygon_file = NULL;
  int web_mercator = 0, location = LOC_NONE, append = 0, have_fields = 0, num_fields = 0, info = 0, auto_offset = 1;
  double z_range[2] = {-1.0 / 0.0, 1.0 / 0.0}, box[6] = {0}, scale = 0.001, offset[3] = {0, 0, 0};
  long zoom = -1, format = -1;
  const char* fields[MAX_FIELDS];
  static uint64_t cells[MAX_CELLS];
  uint32_t num_cells = 0;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    char* end;
    if (strcmp(a, "--help") == 0 || strcmp(a, "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    } else if (strcmp(a, "--aabb") == 0 && more && location == LOC_NONE) {
      if (!parse_doubles(argv[++i], box, 6)) return usage();
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
      if (!parse_doubles(argv[++i], z_range, 2)) return usage();
    } else if (strcmp(a, "--all") == 0 && location == LOC_NONE) {
      location = LOC_ALL;
    } else if (strcmp(a, "--scale") == 0 && more) {
      scale = strtod(argv[++i], &end);
      if (end == argv[i] || *end) return usage();
    } else if (strcmp(a, "--offset") == 0 && more) {
      ++i;
      auto_offset = strcmp(argv[i], "auto") == 0;
      if (!auto_offset && !parse_doubles(argv[i], offset, 3)) return usage();
    } else if (strcmp(a, "--format") == 0 && more) {
      format = strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || format < 0 || format > 10) return usage();
    } else if (strcmp(a, "--fields") == 0 && more && !have_fields) {
      if ((num_fields = split_commas(argv[++i], fields, MAX_FIELDS)) < 0) return usage();
      have_fields = 1;
    } else if (strcmp(a, "--output") == 0 && more && !output) {
      output = argv[++i];
    } else if (strcmp(a, "--per-location") == 0 && more && !pattern) {
      pattern = argv[++i];
      const char* mark = strstr(pattern, "%u");
      if (!mark || strchr(mark + 1, '%') || strchr(pattern, '%') != mark) return usage(); /* exactly one %u, no other % */
    } else if (strcmp(a, "--append") == 0) {
      append = 1;
    } else if (strcmp(a, "--info") == 0) {
      info = 1;
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
  double lo[3], hi[3];
  uint64_t *first = NULL, *seg_offset = NULL;
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

  /* ---- the query ---- */
  what = "query";
  uint64_t num_segments = 0, num_points = 0;
  if (cloud) {
    rc = pcv_s2_query_run_ex(cloud, shapes, num_unions, union_first, cells, NULL, 0, &query);
    if (rc == PCV_OK) rc = pcv_s2_query_sizes(query, &num_segments, &num_points);
  } else {
    rc = pcv_query_batch_run(ctx, shapes, tree, NULL, NULL, &batch);
    if (rc == PCV_OK) rc = pcv_query_batch_sizes(batch, &num_segments, &num_points);
  }
  if (rc != PCV_OK) goto done;

  /* ---- the files ---- */
  what = "write";
  pcv_las_write_params params;
  memset(&params, 0, sizeof(params));
  params.struct_size = (uint32_t)sizeof(params);
  params.open_mode = append ? PCV_LAS_APPEND : PCV_LAS_TRUNCATE;
  params.point_format = format < 0 ? PCV_LAS_FORMAT_AUTO : (uint32_t)format;
  for (int a = 0; a < 3; ++a) params.scale[a] = scale, params.offset[a] = offset[a];
  params.auto_offset = (uint32_t)auto_offset;
  params.fields = have_fields ? fields : NULL;
  params.num_fields = (uint32_t)num_fields;
  pcv_las_write_info written;
  rc = cloud ? pcv_s2_query_write_las(query, 0, num_segments, output, &params, &written)
             : pcv_query_batch_write_las(batch, 0, num_segments, output, &params, &written);
  if (rc != PCV_OK) goto done;
  printf("%s: %u locations, %llu segments, %llu points %s %s\n", dir, locations, (unsigned long long)num_segments,
         (unsigned long long)written.num_records, append ? "appended to" : "written to",
         written.num_records ? output : "no file (a LAS file without points is not written)");
  if (info) print_info(&written);
  if (pattern) {
    first = (uint64_t*)calloc((size_t)locations + 1, sizeof(uint64_t));
    seg_offset = (uint64_t*)calloc((size_t)num_segments + 1, sizeof(uint64_t));
    char* path = (char*)malloc(strlen(pattern) + 16);
    if (!first || !seg_offset || !path) rc = PCV_E_OOM;
    if (rc == PCV_OK) rc = cloud ? pcv_s2_query_segments(query, first, NULL, seg_offset) : pcv_query_batch_segments(batch, first, NULL, seg_offset);
    const size_t mark = (size_t)(strstr(pattern, "%u") - pattern);
    for (uint32_t l = 0; rc == PCV_OK && l < locations; ++l) {
      sprintf(path, "%.*s%u%s", (int)mark, pattern, l, pattern + mark + 2);
      rc = cloud ? pcv_s2_query_write_las(query, first[l], first[l + 1] - first[l], path, &params, &written)
                 : pcv_query_batch_write_las(batch, first[l], first[l + 1] - first[l], path, &params, &written);
      if (rc == PCV_OK && written.num_records) {
        printf("  location %u: %llu points -> %s\n", l, (unsigned long long)written.num_records, path);
        if (info) print_info(&written);
      }
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
  free(seg_offset);
  free(first);
  free(specs);
  return rc == PCV_OK ? 0 : 1;
}
