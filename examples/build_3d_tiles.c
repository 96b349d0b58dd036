/* build_3d_tiles.c — "the points themselves in a globe viewer", in plain C11 on top of the C ABI: an octree directory as an OGC
 * 3D Tiles 1.0 tileset, tileset.json and one Point Cloud (.pnts) file per node that holds points. The octree maps onto the
 * format one to one ("refine":"ADD", a node's cube is the tile's box); the product is stated in include/pcv_hip.h. The call
 * sequence of a non-Python host:
 *   pcv_cloud_kind -> pcv_octree_open_dir -> pcv_tiles3d_plan -> pcv_tiles3d_write_dir
 * The node files are read and uploaded once; every .pnts file is packed on the device.
 *
 *   build_3d_tiles <octree dir> --output-directory D [--error-factor F] [--position-mode auto|quantized|float] [--intensity] [--info]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static const char kUsage[] =
    "usage: build_3d_tiles <octree dir> --output-directory D [--error-factor F] [--position-mode auto|quantized|float] [--intensity] [--info]\n"
    "  <octree dir>          an octree directory (meta.pb and node files); for a globe viewer its points are ECEF\n"
    "  --output-directory    where tileset.json and <NodeId>.pnts go\n"
    "  --error-factor        geometricError of a tile with children = its edge times F (default 0.0625)\n"
    "  --position-mode       auto (default): quantized for u8 / u16 nodes, float for f32 / f64 nodes; or one form for every tile\n"
    "  --intensity           add the INTENSITY batch table (the octree must carry intensity)\n"
    "  --info                also print one line per .pnts file: name, points, mode, bytes\n";

static int usage(void) {
  fputs(kUsage, stderr);
  return 2;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (strcmp(argv[i], "--help") == 0 || strcmp(argv[i], "-h") == 0) {
      fputs(kUsage, stdout);
      return 0;
    }
  const char *dir = NULL, *output = NULL;
  pcv_tiles3d_params params;
  memset(&params, 0, sizeof(params));
  params.error_factor = PCV_TILES3D_DEFAULT_ERROR_FACTOR;
  int info_lines = 0;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const int more = i + 1 < argc;
    if (strcmp(a, "--output-directory") == 0 && more && !output) {
      output = argv[++i];
    } else if (strcmp(a, "--error-factor") == 0 && more) {
      char* end = NULL;
      params.error_factor = strtod(argv[++i], &end);
      if (end == argv[i] || *end) return usage();
    } else if (strcmp(a, "--position-mode") == 0 && more) {
      const char* s = argv[++i];
      if (strcmp(s, "auto") == 0) params.position_mode = PCV_TILES3D_POS_AUTO;
      else if (strcmp(s, "quantized") == 0) params.position_mode = PCV_TILES3D_POS_QUANTIZED;
      else if (strcmp(s, "float") == 0) params.position_mode = PCV_TILES3D_POS_FLOAT;
      else return usage();
    } else if (strcmp(a, "--intensity") == 0) {
      params.flags |= PCV_TILES3D_INTENSITY;
    } else if (strcmp(a, "--info") == 0) {
      info_lines = 1;
    } else if (a[0] != '-' && !dir) {
      dir = a;
    } else {
      return usage();
    }
  }
  if (!dir || !output) return usage();
  if (pcv_tiles3d_check_params_host(&params) != PCV_OK) {
    fprintf(stderr, "%s\n", pcv_host_last_error());
    return usage();
  }

  int kind = 0, rc;
  if ((rc = pcv_cloud_kind(dir, &kind)) != PCV_OK) {
    fprintf(stderr, "cannot open %s (%d): %s\n", dir, rc, pcv_host_last_error());
    return 1;
  }
  if (kind != PCV_CLOUD_OCTREE) {
    fprintf(stderr, "%s is an S2 cell cloud; a tileset is made from an octree\n", dir);
    return 1;
  }
  pcv_ctx* ctx = NULL;
  if ((rc = pcv_ctx_create(0, NULL, &ctx)) != PCV_OK) {
    fprintf(stderr, "no HIP device (pcv_ctx_create: %d); there is no CPU fallback\n", rc);
    return 1;
  }
  pcv_octree* tree = NULL;
  pcv_tiles3d* tiles = NULL;
  pcv_tiles3d_tile* list = NULL;
  const char* what = "open";
  if ((rc = pcv_octree_open_dir(ctx, dir, &tree)) != PCV_OK) goto done;
  what = "plan";
  if ((rc = pcv_tiles3d_plan(tree, &params, &tiles)) != PCV_OK) goto done;
  what = "write";
  if ((rc = pcv_tiles3d_write_dir(tiles, output)) != PCV_OK) goto done;
  pcv_tiles3d_info info;
  pcv_tiles3d_info_get(tiles, &info);
  printf("%s: %llu points in %llu files (%llu bytes), %llu tiles -> %s\n", dir, (unsigned long long)info.points,
         (unsigned long long)info.content_tiles, (unsigned long long)info.total_file_bytes, (unsigned long long)info.tiles, output);
  if (info_lines && info.content_tiles) {
    list = (pcv_tiles3d_tile*)malloc((size_t)info.content_tiles * sizeof(*list));
    if (list && pcv_tiles3d_tiles(tiles, info.content_tiles, list, NULL) == PCV_OK)
      for (uint64_t k = 0; k < info.content_tiles; ++k) {
        pcv_node_info nd;
        char name[64] = "r";
        if (pcv_octree_node(tree, list[k].node, &nd) != PCV_OK) continue;
        for (uint32_t j = 0; j < nd.level && j < 42; ++j) { /* NodeId Display: one octal digit per level, the first level first */
          const uint32_t shift = 3 * (nd.level - 1 - j);
          const uint64_t digit = shift >= 64 ? ((nd.id_high & 0x00ffffffffffffffull) >> (shift - 64))
                                             : (shift > 61 ? (nd.id_low >> shift) | (nd.id_high << (64 - shift)) : nd.id_low >> shift);
          name[1 + j] = (char)('0' + (int)(digit & 7));
          name[2 + j] = 0;
        }
        printf("%s.pnts %llu %s %llu\n", name, (unsigned long long)list[k].num_points,
               list[k].mode == PCV_TILES3D_POS_QUANTIZED ? "quantized" : "float", (unsigned long long)list[k].file_bytes);
      }
  }

done:
  if (rc != PCV_OK) fprintf(stderr, "%s failed (%d): %s\n", what, rc, pcv_last_error(ctx));
  free(list);
  pcv_tiles3d_free(tiles);
  if (tree) pcv_octree_free(tree);
  pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
