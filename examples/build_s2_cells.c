/* build_s2_cells.c — an S2 cell cloud directory from a PLY file of ECEF points, in plain C11 on top of the C ABI: what the
 * reference's S2Splitter (src/read_write/s2.rs) leaves on disk for one batch. The call sequence of a non-Python host:
 *   pcv_ply_read -> pcv_ply_points (host SoA) -> pcv_s2_split (ids, regroup, gather on the device) -> pcv_s2_write_dir
 * Any other source of SoA arrays goes the same way: fill a pcv_points by hand and skip the first two calls.
 * With --batch-points N the arrays go through a directory stream in slices of N points, as a reader that yields batches would
 * feed it (S2Splitter::write once per batch): pcv_s2_stream_begin -> pcv_s2_stream_append ... -> pcv_s2_stream_finish; the device
 * holds the pending batches only, the directory is the same. --append adds to the S2 directory that is there (OpenMode::Append).
 *
 *   build_s2_cells <input.ply> --output-directory <dir> [--split-level 20] [--batch-points N] [--append]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static int usage(void) {
  fprintf(stderr, "usage: build_s2_cells <input.ply> --output-directory <dir> [--split-level 20] [--batch-points N] [--append]\n");
  return 2;
}

int main(int argc, char** argv) {
  const char* input = NULL;
  const char* outdir = NULL;
  long level = 20; /* DEFAULT_S2_SPLIT_LEVEL, s2.rs:17 */
  long long batch_points = 0; /* 0: one pcv_s2_split of the whole file */
  int append = 0;
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--output-directory") == 0 && i + 1 < argc) outdir = argv[++i];
    else if (strcmp(argv[i], "--split-level") == 0 && i + 1 < argc) level = atol(argv[++i]);
    else if (strcmp(argv[i], "--batch-points") == 0 && i + 1 < argc) batch_points = atoll(argv[++i]);
    else if (strcmp(argv[i], "--append") == 0) append = 1;
    else if (argv[i][0] != '-' && !input) input = argv[i];
    else return usage();
  }
  if (!input || !outdir || level < 0 || level > 30 || batch_points < 0) return usage();

  char err[512] = "";
  pcv_ply* ply = NULL;
  pcv_points points;
  if (pcv_ply_read(input, &ply, err, sizeof(err)) != PCV_OK || pcv_ply_points(ply, &points) != PCV_OK) {
    fprintf(stderr, "cannot read %s: %s\n", input, err);
    pcv_ply_free(ply);
    return 1;
  }
  if (!points.color) {
    fprintf(stderr, "%s has no red/green/blue properties; an S2 cell cloud carries the colour attribute\n", input);
    pcv_ply_free(ply);
    return 1;
  }
  pcv_ctx* ctx = NULL;
  int rc;
  if ((rc = pcv_ctx_create(0, NULL, &ctx)) != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    pcv_ply_free(ply);
    return 1;
  }
  pcv_s2_cloud* cloud = NULL;
  if (batch_points == 0 && !append) {
    rc = pcv_s2_split(ctx, &points, (uint32_t)level, &cloud);
    if (rc == PCV_OK) rc = pcv_s2_write_dir(cloud, outdir);
  } else {
    pcv_s2_stream_params params;
    memset(&params, 0, sizeof(params));
    params.struct_size = (uint32_t)sizeof(params);
    params.split_level = (uint32_t)level;
    params.directory = outdir;
    params.open_mode = append ? PCV_S2_APPEND : PCV_S2_TRUNCATE;
    pcv_s2_stream* stream = NULL;
    rc = pcv_s2_stream_begin(ctx, &params, &stream);
    const uint64_t step = batch_points ? (uint64_t)batch_points : points.n;
    for (uint64_t at = 0; rc == PCV_OK && at < points.n; at += step) {
      pcv_points batch = points;
      batch.n = points.n - at < step ? points.n - at : step;
      batch.x += at, batch.y += at, batch.z += at;
      batch.color += at * points.color_stride;
      if (points.intensity) batch.intensity += at;
      rc = pcv_s2_stream_append(stream, &batch);
    }
    if (rc == PCV_OK) rc = pcv_s2_stream_finish(stream, &cloud);
    else pcv_s2_stream_abort(stream);
  }
  if (rc != PCV_OK) {
    fprintf(stderr, "split of %s failed (%d): %s\n", input, rc, pcv_last_error(ctx));
  } else {
    uint64_t cells = 0, n = 0;
    pcv_s2_info(cloud, &cells, &n, NULL, NULL, NULL, NULL);
    printf("%llu points -> %llu level-%ld cells in %s\n", (unsigned long long)n, (unsigned long long)cells, level, outdir);
  }
  pcv_s2_free(cloud);
  pcv_ctx_destroy(ctx);
  pcv_ply_free(ply);
  return rc == PCV_OK ? 0 : 1;
}
