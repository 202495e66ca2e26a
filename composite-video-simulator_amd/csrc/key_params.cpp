// key_params.cpp -- host half of the colorkey stage (include/ntscsim.h: ntscsim_key_*): the tool's switches, the
// layer list, the positions of its rand() draws and the start states of the draw kernel's lanes.  Plain C++: no HIP,
// usable without a GPU.  Line numbers refer to ffmpeg_colorkey.cpp of the reference.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "key_host.hpp"
#include "ntscsim.h"

extern "C" void ntscsim_key_params_init(ntscsim_key_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->width = 720;                      // preset_NTSC() :606-613, called first by main() :889
    p->height = 480;
    p->delay = 1;                        // output_avstream_video_frame_delay :62
}

extern "C" void ntscsim_key_params_free(ntscsim_key_params *p)
{
    if (!p || p->struct_size != sizeof(*p)) return;
    std::free(p->layers);
    p->layers = nullptr;
    p->n_layers = p->layers_cap = 0;
}

extern "C" int ntscsim_key_params_add_layer(ntscsim_key_params *p, const char *path)
{
    if (!p || p->struct_size != sizeof(*p) || p->n_layers < 0 || p->n_layers > p->layers_cap) return NTSCSIM_E_ARG;
    if (p->n_layers == p->layers_cap) {
        const int cap = p->layers_cap ? p->layers_cap * 2 : 4;
        void *m = std::realloc(p->layers, (size_t)cap * sizeof(ntscsim_key_layer));
        if (!m) return NTSCSIM_E_NOMEM;
        p->layers = static_cast<ntscsim_key_layer *>(m);
        p->layers_cap = cap;
    }
    ntscsim_key_layer &l = p->layers[p->n_layers];
    if (p->n_layers > 0) l = p->layers[p->n_layers - 1];                        // new_input_file() :572-581
    else {                                                                      // InputFile() :68
        std::memset(&l, 0, sizeof(l));
        l.xdivr = 1;
    }
    l.path = path;                                                              // reset_on_dup() :90-92
    return p->n_layers++;
}

extern "C" int ntscsim_key_parse_argv(ntscsim_key_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    // current_input_file() :562-569 throws when there is no input yet
    ntscsim_key_layer *cur = p->n_layers > 0 ? &p->layers[p->n_layers - 1] : nullptr;
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :723-726
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "f")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->fade = (unsigned int)std::strtoul(a, nullptr, 0);
        }
        else if (!std::strcmp(a, "d")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            const unsigned int d = (unsigned int)std::strtoul(a, nullptr, 0);
            if (d == 0 || d > 256) return NTSCSIM_E_FLAG;                        // "Invalid delay" :652-655
            p->delay = (int32_t)d;
        }
        else if (!std::strcmp(a, "xd")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->xdivr = (unsigned int)std::strtoul(a, nullptr, 0);
        }
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->width = (int)std::strtoul(a, nullptr, 0);
            if (p->width < 32) return NTSCSIM_E_FLAG;
        }
        else if (!std::strcmp(a, "noise")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->noisekey = (unsigned int)(int)std::strtoul(a, nullptr, 0);
        }
        else if (!std::strcmp(a, "inv")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->invert = (int)std::strtoul(a, nullptr, 0) > 0;
        }
        else if (!std::strcmp(a, "threshhold")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->threshhold = (int)std::strtoul(a, nullptr, 0);
        }
        else if (!std::strcmp(a, "color")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (!cur) return NTSCSIM_E_ARG;
            cur->color = (uint32_t)(int)std::strtoul(a, nullptr, 0);
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            const int rc = ntscsim_key_params_add_layer(p, a);
            if (rc < 0) return rc;
            cur = &p->layers[p->n_layers - 1];
        }
        else if (!std::strcmp(a, "o")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_path = a;
        }
        else if (!std::strcmp(a, "422")) p->use_422_colorspace = 1;
        else if (!std::strcmp(a, "420")) p->use_422_colorspace = 0;
        else if (!std::strcmp(a, "tvstd")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;                          // the tool hands the NULL to strcmp
            if (!std::strcmp(a, "pal")) { p->tv_standard = 1; p->width = 720; p->height = 576; }     // :597-604
            else if (!std::strcmp(a, "ntsc")) { p->tv_standard = 0; p->width = 720; p->height = 480; }
            else return NTSCSIM_E_FLAG;
        }
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :718-721
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :729-736
    if (require_io && p->n_layers == 0) return NTSCSIM_E_FLAG;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_key_rand_advance(const ntscsim_key_params *p, const uint8_t *present, uint64_t *pos)
{
    if (!p || !pos || p->struct_size != sizeof(*p) || p->n_layers < 0 || (p->n_layers > 0 && !p->layers)) return NTSCSIM_E_ARG;
    if (p->width <= 0 || p->height <= 0) return NTSCSIM_E_SIZE;
    const uint64_t per = 3ull * (uint64_t)p->width * (uint64_t)p->height;      // :860-861 inside both loops :844,848
    for (int l = 0; l < p->n_layers; l++)
        if ((!present || present[l]) && p->layers[l].noisekey > 0) *pos += per;  // :837-842 returns before any draw
    return NTSCSIM_OK;
}

namespace ntscsim {

void key_lane_polys(uint32_t lanes, std::vector<uint32_t> &out)
{
    out.assign((size_t)31 * lanes, 0);
    const RandPoly step = rand_poly_pow(KEY_RUN_DRAWS);
    RandPoly cur = rand_poly_one();
    for (uint32_t j = 0; j < lanes; j++) {
        for (int k = 0; k < 31; k++) out[(size_t)k * lanes + j] = cur.c[k];
        cur = rand_poly_mul(cur, step);
    }
}

RandState key_lane_state(const uint32_t *polys, uint32_t lanes, uint32_t lane, const RandState &job)
{
    RandPoly c;
    for (int k = 0; k < 31; k++) c.c[k] = polys[(size_t)k * lanes + lane];
    return rand_state_apply(c, job);
}

} // namespace ntscsim

extern "C" int ntscsim_key_debug_lane_state(int width, int height, uint64_t job_pos, uint32_t lane, uint32_t out[31])
{
    if (!out || width <= 0 || height <= 0) return NTSCSIM_E_ARG;
    const uint32_t lanes = ntscsim::key_lanes_per_job(width, height);
    if (lane >= lanes) return NTSCSIM_E_ARG;
    std::vector<uint32_t> polys;
    ntscsim::key_lane_polys(lanes, polys);
    const ntscsim::RandState s = ntscsim::key_lane_state(polys.data(), lanes, lane, ntscsim::rand_state_at(job_pos));
    std::memcpy(out, s.w, sizeof(s.w));
    return NTSCSIM_OK;
}
