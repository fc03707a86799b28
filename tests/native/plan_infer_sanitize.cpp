// The composed inference plan (csrc/mlp_plan.h: make_plan_infer) compiled for the CPU with -fsanitize=address,undefined and swept
// over the descriptor space, like plan_sanitize.cpp does for the regular plans: every element of every slab of the composed stream
// takes its value from inside the buffer its layer reads (the parameters for the trunk and the rgb head, the composed parameters
// for sigma' and dir-net'), every such value is read, and the trunk and rgb slabs read what the regular stream's slabs read.
#define __host__
#define __device__
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct snerf_mlp_desc {
    int32_t n_layers, width, pos_freqs, pos_identity, dir_freqs, dir_identity, add_dim;
    uint32_t skip_mask;
    int32_t use_dir, add_first;
};
struct snerf_warp_desc {
    int32_t width, pos_freqs, pos_identity, pose_dim;
};
#include "../../smpl_nerf_amd/csrc/mlp_plan.h"

using namespace snerf;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__);   \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static long checked = 0, refused = 0;

static void check_infer_plan(const snerf_mlp_desc &d) {
    Plan R, P;
    const char *why = "";
    if (make_plan(d, R, why, 16) != 0) return;
    if (make_plan_infer(d, P, why) != 0) {
        CHECK(R.width > 256);
        ++refused;
        return;
    }
    ++checked;
    const int nh = R.n_hidden;
    CHECK(R.composed == 0 && P.composed == 1 && P.nlayers == nh + 4 && R.nlayers == nh + 6 && P.width == R.width);
    CHECK(P.param_floats == R.param_floats && P.n_hidden == nh);
    // the trunk: the regular plan's layers, slab for slab
    for (int l = 0; l <= nh; ++l) {
        CHECK(P.layer[l].first_slab == R.layer[l].first_slab && P.layer[l].nslab == R.layer[l].nslab);
        CHECK(P.layer[l].w_off == R.layer[l].w_off && P.layer[l].b_off == R.layer[l].b_off && P.layer[l].nkb == R.layer[l].nkb);
    }
    const Layer &Ls = P.layer[nh + 1], &Ld = P.layer[nh + 2], &Lr = P.layer[nh + 3];
    const int W = d.width, WD = W / 2, dir_dim = d.use_dir ? P.dir_dim : 0;
    CHECK(Ls.n_out == 1 && Ls.n_in == W && Ld.n_out == WD && Ld.n_in == W + dir_dim && Lr.n_out == 3 && Lr.n_in == WD);
    CHECK(Lr.w_off == R.layer[nh + 5].w_off && Lr.b_off == R.layer[nh + 5].b_off);
    CHECK(Ls.w_off == 0 && Ls.b_off == W && Ld.w_off == W + 1 && Ld.b_off == W + 1 + (int64_t)WD * (W + dir_dim));
    CHECK(P.comp_floats == Ld.b_off + WD);
    int slab = R.layer[nh].first_slab + R.layer[nh].nslab;
    for (int l = nh + 1; l < P.nlayers; ++l) {
        CHECK(P.layer[l].first_slab == slab && SLAB_TILES % P.layer[l].t_out == 0);
        const int kps = SLAB_TILES / P.layer[l].t_out;
        CHECK(P.layer[l].nslab == (P.layer[l].nkb + kps - 1) / kps);
        slab += P.layer[l].nslab;
    }
    CHECK(slab == P.total_slabs && P.total_slabs < R.total_slabs);
    // every element of the stream behind the trunk: its source lies in its layer's buffer, and every value of that buffer is read
    std::vector<char> hit_comp((size_t)P.comp_floats, 0), hit_rgb((size_t)(3 * WD + 3), 0);
    for (int l = nh + 1; l < P.nlayers; ++l) {
        const Layer &Ly = P.layer[l];
        for (int sl = 0; sl < Ly.nslab; ++sl)
            for (int e = 0; e < SLAB_FLOATS; ++e) {
                const int64_t src = fwd_slab_src(Ly, sl, e);
                if (src < 0) continue;
                if (l < nh + 3) {
                    CHECK(src < P.comp_floats);
                    ++hit_comp[(size_t)src];
                } else {
                    CHECK(src >= Lr.w_off && src < P.param_floats && src - Lr.w_off < (int64_t)hit_rgb.size());
                    ++hit_rgb[(size_t)(src - Lr.w_off)];
                    // the same element of the regular stream's rgb slab
                    CHECK(fwd_slab_src(R.layer[nh + 5], sl, e) == src);
                }
            }
    }
    for (char h : hit_comp) CHECK(h == 1);
    for (char h : hit_rgb) CHECK(h == 1);
    // the scratch of the pack behind the pad slabs (mlp.hip: infer_scratch) starts 8-byte aligned
    CHECK(((int64_t)(P.total_slabs + SLAB_PAD) * SLAB_FLOATS * 4) % 8 == 0);
}

int main() {
    // (the additional inputs and the skips shape the trunk, which is the regular plan's: two settings of each)
    for (int n_layers : {1, 2, 8, 16})
        for (int width : {2, 7, 30, 64, 100, 128, 200, 250, 256, 320, 512})
            for (int pL : {0, 10})
                for (int pid = 0; pid < 2; ++pid)
                    for (int dL : {0, 4, 16})
                        for (int add : {0, 69})
                            for (uint32_t skip : {0u, (1u << 0) | (1u << 4)})
                                for (int use_dir = 0; use_dir < 2; ++use_dir)
                                    for (int add_first = 0; add_first < (add ? 2 : 1); ++add_first) {
                                        snerf_mlp_desc d{n_layers, width, pL, pid, dL, 1 - pid, add, skip & ((1u << (n_layers - 1)) - 1u),
                                                         use_dir, add_first};
                                        check_infer_plan(d);
                                    }
    // the default net: 60 + 1 + 5 + 1 slabs
    {
        snerf_mlp_desc d{8, 256, 10, 0, 4, 0, 0, 1u << 4, 1, 0};
        Plan P;
        const char *why = "";
        CHECK(make_plan_infer(d, P, why) == 0 && P.total_slabs == 67);
    }
    std::printf("inference plans checked: %ld, refused above width 256: %ld\n", checked, refused);
    return (checked > 2000 && refused > 100) ? 0 : 2;
}
