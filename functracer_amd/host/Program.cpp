// Program.cpp — command-line driver with the flow of Program.fs:51-100: parse the scene,
// create the image plane + rays + shade + blend (one ft_render call on the GPU), write the PNG.
//   functracer <scene-file> [output.png]        (2 args: file output; otherwise PNG to stdout)
//   functracer <scene-file> <output.png> --denoise N
//                                               the frame filtered on the device before it is written: ft_denoise with N a-trous
//                                               iterations (0 .. 6) guided by the surfaces of sample 0, demodulated by the material colour;
//                                               sigma_colour 0.6, sigma_normal 0.3, sigma_position 0 (off), albedo_floor 1e-3, no variance
//   functracer <scene-file> --intersection-at X Y
//                                               what is at pixel (X, Y), row 0 = top, on stderr; no image (the device counterpart of
//                                               printIntersectionAt, Program.fs:33-49: ft_render_aov of a 1x1 tile, jitter offset (0, 0))
// Phase timings go to stderr like the reference's eprintfn calls (Program.fs:53-67).  Unlike the
// reference nothing but the PNG is ever written to stdout (its printfn calls at Program.fs:96-97
// corrupt the PNG stream the GUI reads).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_api.h"

static const fth_builder kHipBuilder = {
    [](void* c, int32_t k) { return ft_sg_primitive((ft_context*)c, k); },
    [](void* c, const double* v) { return ft_sg_triangle((ft_context*)c, v); },
    [](void* c, int32_t d, const double* t, int64_t n) { return ft_sg_bsp_mesh((ft_context*)c, d, t, n); },
    [](void* c, const ft_transform* ts, int32_t n, ft_node ch) { return ft_sg_transform((ft_context*)c, ts, n, ch); },
    [](void* c, const ft_material* m, ft_node ch) { return ft_sg_material((ft_context*)c, m, ch); },
    [](void* c, double a, ft_node ch) { return ft_sg_hue_shift((ft_context*)c, a, ch); },
    [](void* c, ft_node ch) { return ft_sg_ignore_light((ft_context*)c, ch); },
    [](void* c, const ft_node* ch, int32_t n) { return ft_sg_group((ft_context*)c, ch, n); },
    [](void* c, int32_t op, ft_node a, ft_node b) { return ft_sg_csg((ft_context*)c, op, a, b); },
    [](void* c, const double* ca, const double* cb, const double* ops, int32_t n, ft_node ch) { return ft_sg_texture_grid((ft_context*)c, ca, cb, ops, n, ch); },
    [](void* c, const uint8_t* px, int32_t w, int32_t h, const double* ops, int32_t n, ft_node ch) { return ft_sg_texture_image((ft_context*)c, px, w, h, ops, n, ch); },
    [](void* c) { return ft_scene_clear((ft_context*)c); },
    [](void* c, ft_node r) { return ft_scene_set_objects((ft_context*)c, r); },
    [](void* c, const double* d, const double* col) { return ft_scene_add_directional((ft_context*)c, d, col); },
    [](void* c, const double* d, int32_t s, double sc, const double* col) { return ft_scene_add_soft_directional((ft_context*)c, d, s, sc, col); },
    [](void* c, const double* p, const double* f, const double* col) { return ft_scene_add_positional((ft_context*)c, p, f, col); },
    [](void* c) { return ft_scene_commit((ft_context*)c); },
};

// The hit record of one pixel (ft_render_aov over a 1x1 tile), printed as `key = value` lines; doubles round-trip (%.17g).
static int print_intersection_at(ft_context* ctx, const fth_options& opt, int32_t x, int32_t y, uint64_t seed) {
    if (x < 0 || y < 0 || x >= opt.res_h || y >= opt.res_v) { std::fprintf(stderr, "pixel (%d, %d) outside the %dx%d image\n", x, y, opt.res_h, opt.res_v); return 1; }
    const size_t n = (size_t)opt.res_h * opt.res_v, at = (size_t)y * opt.res_h + x;
    std::vector<double> t(n), p(3 * n), nr(3 * n), col(3 * n), mat(3 * n);
    std::vector<int32_t> leaf(n, -1), node(n, -1), tri(n, -1);
    const ft_aov aov{t.data(), p.data(), nr.data(), col.data(), mat.data(), leaf.data(), node.data(), tri.data()};
    const double jitter[2] = {0.0, 0.0};
    const ft_rect px{x, y, 1, 1};
    const int32_t rc = ft_render_aov(ctx, &opt.camera, opt.res_h, opt.res_v, 1, jitter, 0, seed, &px, 1, &aov, nullptr);
    if (rc != FT_OK) { std::fprintf(stderr, "ft_render_aov failed (%d): %s\n", rc, ft_last_error(ctx)); return 1; }
    std::fprintf(stderr, "intersection at (%d, %d):\n", x, y);
    if (leaf[at] < 0) { std::fprintf(stderr, "None\n"); return 0; }
    auto v3 = [&](const char* k, const std::vector<double>& v) { std::fprintf(stderr, "%s = %.17g %.17g %.17g\n", k, v[3 * at], v[3 * at + 1], v[3 * at + 2]); };
    std::fprintf(stderr, "t = %.17g\n", t[at]);
    v3("p", p); v3("n", nr); v3("colour", col); v3("material", mat);
    std::fprintf(stderr, "leaf = %d\nnode = %d\ntriangle = %d\n", leaf[at], node[at], tri[at]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: functracer <scene-file> [output.png | --intersection-at X Y]\n"); return 2; }
    const bool pick = argc >= 3 && std::strcmp(argv[2], "--intersection-at") == 0;
    if (pick && argc != 5) { std::fprintf(stderr, "usage: functracer <scene-file> --intersection-at X Y\n"); return 2; }
    const bool denoise = argc >= 4 && std::strcmp(argv[3], "--denoise") == 0;
    if (denoise && argc != 5) { std::fprintf(stderr, "usage: functracer <scene-file> <output.png> --denoise N\n"); return 2; }
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count(); };
    std::fprintf(stderr, "Using input file: %s\n", argv[1]);
    char err[1024] = {0};
    fth_scene* scene = fth_parse_scene_file(argv[1], err, sizeof err);
    if (!scene) { std::fprintf(stderr, "%s\n", err); return 1; }                 // readScene: message + exit 1 (Program.fs:10-16)
    std::fprintf(stderr, "Parsed input %lims\n", ms());
    fth_options opt;
    fth_scene_options(scene, &opt);
    if (opt.corner && !pick) { std::fprintf(stderr, "samples corner (Image.fs:125-150) is not on the device path yet\n"); return 1; }

    int32_t dev = 0;
    if (const char* e = std::getenv("FT_DEVICE")) dev = std::atoi(e);
    ft_context* ctx = nullptr;
    int32_t rc = ft_create(&dev, 1, &ctx);
    if (rc != FT_OK) { std::fprintf(stderr, "ft_create failed (%d): no usable HIP device; this program has no CPU path\n", rc); return 1; }
    rc = fth_scene_lower(scene, &kHipBuilder, ctx);
    if (rc != FT_OK) { std::fprintf(stderr, "scene upload failed (%d): %s\n", rc, ft_last_error(ctx)); return 1; }
    std::fprintf(stderr, "Geometry created %lims\n", ms());

    uint64_t seed = 20260104ull;
    if (const char* e = std::getenv("FT_SEED")) seed = std::strtoull(e, nullptr, 10);
    if (pick) {
        const int prc = print_intersection_at(ctx, opt, std::atoi(argv[3]), std::atoi(argv[4]), seed);
        ft_destroy(ctx);
        fth_scene_free(scene);
        return prc;
    }
    std::vector<double> jitter(2 * (size_t)opt.samples);
    fth_jitter_pattern(seed, opt.samples, jitter.data());
    std::vector<double> rgb((size_t)opt.res_h * opt.res_v * 3);
    ft_stats st;
    rc = ft_render(ctx, &opt.camera, opt.res_h, opt.res_v, opt.samples, jitter.data(), 8, seed, nullptr, 0, rgb.data(), &st);
    if (rc != FT_OK) { std::fprintf(stderr, "ft_render failed (%d): %s\n", rc, ft_last_error(ctx)); return 1; }
    std::fprintf(stderr, "Shaded scene %lims (%.3f ms on the GPU, %.1f Mrays/s, %llu rays)\n", ms(), st.kernel_ms,
                 (double)st.rays_traced / (st.kernel_ms * 1e3), (unsigned long long)st.rays_traced);
    std::vector<uint8_t> rgba((size_t)opt.res_h * opt.res_v * 4);
    if (denoise) {                                                 // the frame is still in HBM: filter it there, bytes out
        const ft_denoise_params dp{std::atoi(argv[4]), 1, 0, 0, 0.6, 0.3, 0.0, 1e-3, 1e-4};
        ft_stats ds;
        rc = ft_denoise(ctx, &opt.camera, opt.res_h, opt.res_v, opt.samples, jitter.data(), 0, seed, nullptr, 0, &dp, 1, rgba.data(), &ds);
        if (rc != FT_OK) { std::fprintf(stderr, "ft_denoise failed (%d): %s\n", rc, ft_last_error(ctx)); return 1; }
        std::fprintf(stderr, "Denoised %lims (%d iterations, %.3f ms on the GPU)\n", ms(), dp.iterations, ds.kernel_ms);
    } else ft_quantise_rgba8(rgb.data(), (int64_t)opt.res_h * opt.res_v, rgba.data());
    std::fprintf(stderr, "Writing output %lims\n", ms());
    const char* out = argc >= 3 ? argv[2] : "/dev/stdout";
    if (argc >= 3) std::fprintf(stderr, "Using output file: %s\n", argv[2]); else std::fprintf(stderr, "Using standard output\n");
    rc = fth_write_png(out, rgba.data(), opt.res_h, opt.res_v);
    ft_destroy(ctx);
    fth_scene_free(scene);
    std::fprintf(stderr, "Elapsed Time: %lims\n", ms());
    return rc == FT_OK ? 0 : 1;
}
