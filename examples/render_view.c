/* render_view.c — one frame of the viewer over the C ABI in plain C11: an octree directory is opened, one camera goes to
 * pcv_render_views (the draw loop of sdl_viewer/src/lib.rs:158-209 on the device), and the frame is written as a PNG.
 *
 *   render_view <octree dir> --matrix <16 doubles> --size WxH [--point-size s] [--gamma g] [--max-nodes n]
 *               [--show-octree-nodes] -o out.png
 *   render_view <octree dir> --look-at <eye xyz> <target xyz> <fovy radians> --size WxH [...]
 *               [--terrain <terrain dir>]... [--terrain-window N] -o out.png
 *
 * --matrix: world_to_gl, column-major, as the viewer uploads it. --look-at: a right-handed look-at view with +z up (+y when
 * looking along z) under Perspective3::new(W / H, fovy, near, far), far = the distance to the farthest corner of the octree's
 * bounding box, near = far / 10 000. --show-octree-nodes: the viewer's `O` key, the yellow wireframe of every drawn node's cube
 * (pcv_render_views_ex with PCV_RENDER_OUTLINE_NODES). Prints "<nodes visible> <nodes drawn> <points submitted> <points drawn>
 * <pixels covered>", and with outlines " <segments submitted> <segments drawn> <outline pixels>" after them.
 * --terrain (repeatable, with --look-at: the eye is the camera position): a terrain directory as sdl_viewer --terrain takes
 * it, drawn after the nodes as the viewer's wireframe layer in a window of --terrain-window vertices (even, 2 ..= 1024, default
 * 1024) around the camera (pcv_terrain_open_dir, pcv_render_views_terrain); per layer " <edges submitted> <edges drawn>
 * <pixels won>" is printed after the rest.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pcv_layout_check.h"

static void look_at(const double eye[3], const double target[3], double fovy, double aspect, const double bmin[3], const double bmax[3],
                    double m[16]) {
  double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
  const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  for (int a = 0; a < 3; ++a) f[a] /= fl;
  const double up[3] = {0.0, fabs(f[2]) > 0.999 ? 1.0 : 0.0, fabs(f[2]) > 0.999 ? 0.0 : 1.0};
  double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  const double sl = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
  for (int a = 0; a < 3; ++a) s[a] /= sl;
  const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
  double far = 0.0;
  for (int c = 0; c < 8; ++c) {
    const double dx = ((c & 1) ? bmax[0] : bmin[0]) - eye[0], dy = ((c & 2) ? bmax[1] : bmin[1]) - eye[1],
                 dz = ((c & 4) ? bmax[2] : bmin[2]) - eye[2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    far = d > far ? d : far;
  }
  const double near = far / 10000.0, t = tan(fovy / 2.0);
  /* rows of the view matrix, then P * V with P = Perspective3::new */
  const double v[4][4] = {{s[0], s[1], s[2], -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2])},
                          {u[0], u[1], u[2], -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2])},
                          {-f[0], -f[1], -f[2], f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]},
                          {0.0, 0.0, 0.0, 1.0}};
  const double p00 = 1.0 / (aspect * t), p11 = 1.0 / t, p22 = (far + near) / (near - far), p23 = 2.0 * far * near / (near - far);
  for (int c = 0; c < 4; ++c) {
    m[4 * c + 0] = p00 * v[0][c];
    m[4 * c + 1] = p11 * v[1][c];
    m[4 * c + 2] = p22 * v[2][c] + p23 * v[3][c];
    m[4 * c + 3] = -v[2][c];
  }
}

int main(int argc, char** argv) {
  const char* usage =
      "usage: render_view <octree dir> --matrix <16 doubles> | --look-at <eye xyz> <target xyz> <fovy> --size WxH "
      "[--point-size s] [--gamma g] [--max-nodes n] [--show-octree-nodes] [--terrain <dir>]... [--terrain-window N] -o out.png\n";
  enum { kMaxTerrain = 16 };
  const char* terrain_dirs[kMaxTerrain];
  pcv_terrain* terrains[kMaxTerrain] = {NULL};
  pcv_render_terrain_layers layers = {0, PCV_RENDER_TERRAIN_WINDOW, terrains, NULL};
  double matrix[16], eye[3] = {0, 0, 0}, target[3] = {0, 0, 0}, fovy = 0.0;
  int have_matrix = 0, have_look = 0;
  pcv_render_params params;
  memset(&params, 0, sizeof(params));
  params.point_size = 1.0f;
  params.gamma = 1.0f;
  pcv_render_overlay overlay = {0, PCV_RENDER_OUTLINE_YELLOW};
  const char* out = NULL;
  if (argc < 2) {
    fputs(usage, stderr);
    return 2;
  }
  for (int i = 2; i < argc; ++i) {
    if (strcmp(argv[i], "--matrix") == 0 && i + 16 < argc) {
      for (int k = 0; k < 16; ++k) matrix[k] = strtod(argv[++i], NULL);
      have_matrix = 1;
    } else if (strcmp(argv[i], "--look-at") == 0 && i + 7 < argc) {
      for (int k = 0; k < 3; ++k) eye[k] = strtod(argv[++i], NULL);
      for (int k = 0; k < 3; ++k) target[k] = strtod(argv[++i], NULL);
      fovy = strtod(argv[++i], NULL);
      have_look = 1;
    } else if (strcmp(argv[i], "--size") == 0 && i + 1 < argc) {
      if (sscanf(argv[++i], "%ux%u", &params.width, &params.height) != 2) params.width = params.height = 0;
    } else if (strcmp(argv[i], "--point-size") == 0 && i + 1 < argc) {
      params.point_size = strtof(argv[++i], NULL);
    } else if (strcmp(argv[i], "--gamma") == 0 && i + 1 < argc) {
      params.gamma = strtof(argv[++i], NULL);
    } else if (strcmp(argv[i], "--max-nodes") == 0 && i + 1 < argc) {
      params.max_nodes = (uint32_t)strtoul(argv[++i], NULL, 10);
    } else if (strcmp(argv[i], "--show-octree-nodes") == 0) {
      overlay.flags |= PCV_RENDER_OUTLINE_NODES;
    } else if (strcmp(argv[i], "--terrain") == 0 && i + 1 < argc && layers.num_layers < kMaxTerrain) {
      terrain_dirs[layers.num_layers++] = argv[++i];
    } else if (strcmp(argv[i], "--terrain-window") == 0 && i + 1 < argc) {
      layers.window = (uint32_t)strtoul(argv[++i], NULL, 10);
    } else if (strcmp(argv[i], "-o") == 0 && i + 1 < argc) {
      out = argv[++i];
    } else {
      fputs(usage, stderr);
      return 2;
    }
  }
  if (have_matrix == have_look || !out || pcv_render_check_params(&params) != PCV_OK) {
    fputs(usage, stderr);
    return 2;
  }
  {  /* the window is checked before any device work, layers or not; the layers themselves are opened below */
    char why[128];
    pcv_render_terrain_layers probe = layers;
    probe.camera_positions = eye;
    probe.num_layers = layers.num_layers ? layers.num_layers : 1;
    for (uint32_t k = 0; k < probe.num_layers; ++k) terrains[k] = (pcv_terrain*)terrain_dirs;  /* not null; never read by the check */
    const int bad = pcv_render_check_terrain_host(&probe, why, sizeof(why));
    for (uint32_t k = 0; k < probe.num_layers; ++k) terrains[k] = NULL;
    if (bad != PCV_OK || (layers.num_layers && !have_look)) {
      fprintf(stderr, "render_view: %s\n", bad != PCV_OK ? why : "--terrain needs --look-at: the eye is the camera position");
      fputs(usage, stderr);
      return 2;
    }
  }
  pcv_ctx* ctx = NULL;
  pcv_octree* tree = NULL;
  pcv_shapes* frusta = NULL;
  pcv_render* frame = NULL;
  uint8_t* rgba = NULL;
  uint8_t* png = NULL;
  int rc = pcv_ctx_create(0, NULL, &ctx);
  if (rc == PCV_OK) rc = pcv_octree_open_dir(ctx, argv[1], &tree);
  if (rc == PCV_OK) {
    pcv_shape shape;
    memset(&shape, 0, sizeof(shape));
    shape.kind = PCV_SHAPE_FRUSTUM;
    if (have_look) {
      double res, bmin[3], bmax[3];
      int version;
      pcv_octree_meta(tree, &res, bmin, bmax, &version);
      look_at(eye, target, fovy, (double)params.width / (double)params.height, bmin, bmax, matrix);
    }
    memcpy(shape.params, matrix, sizeof(matrix));
    rc = pcv_shapes_create(ctx, &shape, 1, &frusta);
  }
  for (uint32_t k = 0; k < layers.num_layers && rc == PCV_OK; ++k) rc = pcv_terrain_open_dir(ctx, terrain_dirs[k], &terrains[k]);
  layers.camera_positions = eye;
  if (rc == PCV_OK) rc = pcv_render_views_terrain(ctx, frusta, tree, &params, &overlay, &layers, &frame);
  int32_t status = 0;
  uint32_t visible = 0, drawn_nodes = 0;
  uint64_t submitted = 0, drawn = 0, covered = 0, need = 0, seg_submitted = 0, seg_drawn = 0, outline_pixels = 0;
  if (rc == PCV_OK) rc = pcv_render_info(frame, 0, &status, &visible, &drawn_nodes, &submitted, &drawn, &covered);
  if (rc == PCV_OK) rc = pcv_render_outline_info(frame, 0, &seg_submitted, &seg_drawn, &outline_pixels);
  if (rc == PCV_OK && status != 0) fprintf(stderr, "render_view: the matrix is not a camera (status %d): the frame is empty\n", (int)status);
  if (rc == PCV_OK) {
    rgba = (uint8_t*)malloc((size_t)4 * params.width * params.height);
    rc = rgba ? pcv_render_images(frame, 0, 1, rgba, PCV_MEM_HOST) : PCV_E_OOM;
  }
  if (rc == PCV_OK) rc = pcv_xray_png_encode(rgba, params.width, params.height, NULL, 0, &need);
  if (rc == PCV_OK) {
    png = (uint8_t*)malloc((size_t)need);
    rc = png ? pcv_xray_png_encode(rgba, params.width, params.height, png, need, &need) : PCV_E_OOM;
  }
  if (rc == PCV_OK) {
    FILE* f = fopen(out, "wb");
    if (!f || fwrite(png, 1, (size_t)need, f) != (size_t)need) rc = PCV_E_IO;
    if (f && fclose(f) != 0) rc = PCV_E_IO;
  }
  if (rc == PCV_OK) {
    printf("%u %u %llu %llu %llu", visible, drawn_nodes, (unsigned long long)submitted, (unsigned long long)drawn, (unsigned long long)covered);
    if (overlay.flags & PCV_RENDER_OUTLINE_NODES)
      printf(" %llu %llu %llu", (unsigned long long)seg_submitted, (unsigned long long)seg_drawn, (unsigned long long)outline_pixels);
    for (uint32_t k = 0; k < layers.num_layers && rc == PCV_OK; ++k) {
      uint64_t edges_submitted = 0, edges_drawn = 0, pixels_won = 0;
      rc = pcv_render_terrain_info(frame, 0, k, NULL, &edges_submitted, &edges_drawn, &pixels_won);
      printf(" %llu %llu %llu", (unsigned long long)edges_submitted, (unsigned long long)edges_drawn, (unsigned long long)pixels_won);
    }
    printf("\n");
  }
  if (rc != PCV_OK)
    fprintf(stderr, "render_view: %s (%d)\n", ctx && rc != PCV_E_IO ? pcv_last_error(ctx) : "cannot write the PNG", rc);
  free(png);
  free(rgba);
  pcv_render_free(frame);
  for (uint32_t k = 0; k < layers.num_layers; ++k) pcv_terrain_free(terrains[k]);
  pcv_shapes_free(frusta);
  if (tree) pcv_octree_free(tree);
  if (ctx) pcv_ctx_destroy(ctx);
  return rc == PCV_OK ? 0 : 1;
}
