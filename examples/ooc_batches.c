/* ooc_batches.c — the reference's `build_octree(dir, resolution, bounding_box, input, attributes)` (src/octree/generation.rs:
 * 289-295) for a cloud larger than the device, over the C ABI in plain C11: PointsBatches of 500 000 points (src/lib.rs:52) go to
 * pcv_ooc_append one at a time as they are (positions AoS, colour, intensity); pcv_ooc_finish builds the tree partition by
 * partition of at most `per_pass` points and writes the directory. The cloud is read from one raw file here — n x 3 f64
 * positions, then n x 3 u8 colours, then n f32 intensities — a real host would hand over whatever its reader produced.
 *
 *   ooc_batches <cloud.bin> <n> <dir> <resolution> <max_points_per_node> <per_pass> <min x y z> <max x y z>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

int main(int argc, char** argv) {
  if (argc < 13) {
    fprintf(stderr, "usage: ooc_batches <cloud.bin> <n> <dir> <resolution> <max_points_per_node> <per_pass> <min x y z> <max x y z>\n");
    return 2;
  }
  const unsigned long long n = strtoull(argv[2], NULL, 10), batch = 500000;
  pcv_build_params params;
  memset(&params, 0, sizeof(params));
  params.resolution = atof(argv[4]);
  params.max_points_per_node = (uint32_t)strtoul(argv[5], NULL, 10);
  const unsigned long long per_pass = strtoull(argv[6], NULL, 10);
  for (int a = 0; a < 3; ++a) params.bbox_min[a] = atof(argv[7 + a]), params.bbox_max[a] = atof(argv[10 + a]);
  FILE* fx = fopen(argv[1], "rb");
  FILE* fc = fopen(argv[1], "rb");
  FILE* fi = fopen(argv[1], "rb");
  if (!fx || !fc || !fi || fseek(fc, (long)(n * 24), SEEK_SET) || fseek(fi, (long)(n * 27), SEEK_SET)) {
    fprintf(stderr, "cannot open the input\n");
    return 1;
  }
  /* one batch of host memory on the input side, whatever the size of the cloud */
  double* xyz = (double*)malloc((size_t)batch * 3 * sizeof(double));
  unsigned char* rgb = (unsigned char*)malloc((size_t)batch * 3);
  float* inten = (float*)malloc((size_t)batch * sizeof(float));
  pcv_ctx* ctx = NULL;
  pcv_ooc* ooc = NULL;
  int rc = pcv_ctx_create(0, NULL, &ctx);
  if (rc != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    return 1;
  }
  rc = pcv_ooc_begin(ctx, &params, 1 /* intensity */, per_pass, &ooc);
  for (unsigned long long at = 0; rc == PCV_OK && at < n; at += batch) {
    const size_t m = (size_t)(n - at < batch ? n - at : batch);
    if (fread(xyz, 3 * sizeof(double), m, fx) != m || fread(rgb, 3, m, fc) != m || fread(inten, sizeof(float), m, fi) != m) {
      fprintf(stderr, "short read at point %llu\n", at);
      rc = PCV_E_IO;
      break;
    }
    rc = pcv_ooc_append(ooc, xyz, rgb, inten, m);
  }
  pcv_ooc_stats st;
  memset(&st, 0, sizeof(st));
  if (rc == PCV_OK) {
    rc = pcv_ooc_finish(ooc, argv[3], &st); /* consumes the handle */
  } else if (ooc) {
    pcv_ooc_abort(ooc);
  }
  if (rc != PCV_OK)
    fprintf(stderr, "build failed (%d): %s\n", rc, pcv_last_error(ctx));
  else
    printf("%llu points -> %llu nodes in %s, %llu partitions, %.1f MB spilled\n", (unsigned long long)st.points, (unsigned long long)st.nodes,
           argv[3], (unsigned long long)st.partitions, st.spill_bytes / 1e6);
  pcv_ctx_destroy(ctx);
  free(xyz);
  free(rgb);
  free(inten);
  fclose(fx);
  fclose(fc);
  fclose(fi);
  return rc == PCV_OK ? 0 : 1;
}
