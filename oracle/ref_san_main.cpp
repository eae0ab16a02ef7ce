// Stand-alone driver of the reference build for `make -C oracle ref_san`: reads the dense and ragged scenes of
// tests/ref_scenes.py from the raw file its write_raw() makes and runs each forward and backward through the reference's own
// kernels (copied sources + ref_shim/ + ref_entry.cpp), everything compiled with -fsanitize=undefined,address,
// float-cast-overflow -fno-sanitize-recover=all.  An index out of its array or an undefined operation in the reference's
// code, in the execution model or in the wrapper ends this program.  Run by hand on a CPU; never from pytest, never loaded
// into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/olsr.h"

extern "C" {
void* ref_create();
void ref_destroy(void* h);
int ref_tile();
int ref_language_channels();
int ref_forward(void* h, const olsr_scene* s, float* out_color, float* out_language, float* out_depth, float* out_opacity,
                int32_t* radii, int32_t* n_touched, int32_t* num_rendered);
int ref_backward(void* h, const olsr_scene* s, const int32_t* radii, const float* dL_dout_color,
                 const float* dL_dout_language, const float* dL_dout_depth, float* dL_dmeans2D, float* dL_dconic,
                 float* dL_dopacity, float* dL_dcolors, float* dL_dlanguage, float* dL_ddepths, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, float* dL_dtau);
}

static FILE* g_f;
static void need(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "ref_san_main: %s\n", what);
    std::exit(2);
  }
}
static std::vector<float> floats(size_t n) {
  std::vector<float> v(n);
  need(n == 0 || std::fread(v.data(), 4, n, g_f) == n, "short read");
  return v;
}

int main(int argc, char** argv) {
  need(argc == 2, "usage: ref_san_main <file written by tests/ref_scenes.py>");
  g_f = std::fopen(argv[1], "rb");
  need(g_f != nullptr, "cannot open the scene file");
  int32_t count = 0;
  need(std::fread(&count, 4, 1, g_f) == 1 && count > 0, "no scene count");
  long runs = 0, rendered = 0;
  double checksum = 0.0;
  for (int32_t k = 0; k < count; ++k) {
    int32_t h[9];
    float tans[2];
    need(std::fread(h, 4, 9, g_f) == 9 && std::fread(tans, 4, 2, g_f) == 2, "short header");
    const size_t P = (size_t)h[0], M = (size_t)h[2], F = (size_t)h[3], W = (size_t)h[4], H = (size_t)h[5];
    const bool has_colors = h[7] != 0, has_cov = h[8] != 0;
    need(h[0] > 0 && h[0] <= 4096 && W * H <= 65536 && M <= 16, "implausible header");
    need(h[6] == ref_tile() && (F == 0 || (int)F == ref_language_channels()), "scene does not fit this build");
    std::vector<float> bg = floats(3), means = floats(3 * P), colors_or_sh = floats(has_colors ? 3 * P : 3 * M * P),
                       lang = floats(F * P), op = floats(P), scales = floats(has_cov ? 0 : 3 * P),
                       rots = floats(has_cov ? 0 : 4 * P), cov = floats(has_cov ? 6 * P : 0), view = floats(16),
                       proj = floats(16), proj_raw = floats(16), campos = floats(3), dc = floats(3 * W * H),
                       dl = floats(F * W * H), dd = floats(W * H);
    olsr_scene s = {};
    s.P = h[0]; s.D = h[1]; s.M = has_colors ? 0 : h[2]; s.F = h[3]; s.width = h[4]; s.height = h[5]; s.tile = h[6];
    s.tan_fovx = tans[0]; s.tan_fovy = tans[1]; s.scale_modifier = 1.0f;
    s.background = bg.data(); s.means3D = means.data();
    s.shs = has_colors ? nullptr : colors_or_sh.data();
    s.colors_precomp = has_colors ? colors_or_sh.data() : nullptr;
    s.language_precomp = F ? lang.data() : nullptr;
    s.opacities = op.data();
    s.scales = has_cov ? nullptr : scales.data(); s.rotations = has_cov ? nullptr : rots.data();
    s.cov3D_precomp = has_cov ? cov.data() : nullptr;
    s.viewmatrix = view.data(); s.projmatrix = proj.data(); s.projmatrix_raw = proj_raw.data(); s.cam_pos = campos.data();
    // every array exactly as long as the binding allocates it: one element past an end is an error here
    std::vector<float> color(3 * W * H), olang(F * W * H), depth(W * H), opac(W * H);
    std::vector<int32_t> radii(P), touched(P);
    std::vector<float> g2(3 * P), gc(4 * P), go(P), gcol(3 * P), gl(F * P), gd(P), g3(3 * P), gcov(6 * P),
        gsh(3 * (has_colors ? 0 : M) * P), gs(3 * P), gr(4 * P), gt(6 * P);
    void* st = ref_create();
    int32_t R = -1;
    need(ref_forward(st, &s, color.data(), olang.data(), depth.data(), opac.data(), radii.data(), touched.data(), &R) == 0,
         "ref_forward failed");
    need(R > 0, "nothing rendered");
    need(ref_backward(st, &s, radii.data(), dc.data(), dl.data(), dd.data(), g2.data(), gc.data(), go.data(), gcol.data(),
                      gl.data(), gd.data(), g3.data(), gcov.data(), gsh.data(), gs.data(), gr.data(), gt.data()) == 0,
         "ref_backward failed");
    ref_destroy(st);
    for (float v : color) checksum += v;
    for (float v : g3) checksum += v;
    rendered += R;
    ++runs;
  }
  std::fclose(g_f);
  std::printf("ref_san_main: %d scenes, %ld forward + backward runs clean (%ld instances, checksum %.9g)\n", (int)count, runs,
              rendered, checksum);
  return 0;
}
