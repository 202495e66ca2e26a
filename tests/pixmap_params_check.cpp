// pixmap_params_check -- csrc/pixmap_params.cpp driven as a stand-alone program: the argument vectors of
// tests/test_pixmap_params.py through ntscsim_post_parse_argv() and ntscsim_cmap_parse_argv(), with the NULL behind
// argv[argc - 1] that main() gets, then ntscsim_pixmap_params_free().  Built plain and with the address and
// undefined-behaviour sanitizers by tests/test_pixmap_params_host.py; prints what it checked and "<n> bad".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ntscsim.h"

struct Case {
    std::vector<const char *> flags;
    int require_io;
    int post, cmap;                      // expected return codes
    int n_layers;                        // where a parse succeeds
    int last_threshhold;                 // of the posterize parse, -1000: not looked at
};

static int bad = 0;

static void expect(bool ok, const char *what, size_t index)
{
    if (!ok) {
        std::printf("case %zu: %s\n", index, what);
        bad++;
    }
}

int main()
{
    const int OK = NTSCSIM_OK, FLAG = NTSCSIM_E_FLAG, HELP = NTSCSIM_E_HELP;
    const std::vector<Case> cases = {
        {{}, 0, OK, OK, 0, -1000},
        {{}, 1, FLAG, FLAG, 0, -1000},
        {{"-i", "a"}, 0, OK, OK, 1, 3},
        {{"-i", "a"}, 1, FLAG, FLAG, 0, -1000},
        {{"-o", "b"}, 1, FLAG, FLAG, 0, -1000},
        {{"-o", "b", "-i", "a"}, 1, OK, OK, 1, 3},
        {{"-i", "a", "-threshhold", "5", "-i", "b", "-i", "c", "-threshhold", "0x2", "-i", "d"}, 0, OK, FLAG, 4, 2},
        {{"-i", "a", "-i", "b", "-i", "c", "-i", "d", "-i", "e", "-i", "f", "-i", "g", "-i", "h", "-i", "i", "-threshhold", "7"}, 0, OK, FLAG, 9, 7},
        {{"-i", "a", "-i", "b", "-i", "c", "-i", "d", "-i", "e"}, 0, OK, OK, 5, 3},
        {{"-threshhold", "5", "-i", "a"}, 0, FLAG, FLAG, 0, -1000},
        {{"-i", "a", "-threshhold"}, 0, FLAG, FLAG, 0, -1000},
        {{"-i", "a", "-threshhold", "9"}, 0, OK, FLAG, 1, 9},
        {{"-i", "a", "-threshhold", "-1"}, 0, OK, FLAG, 1, -1},
        {{"-tvstd", "pal"}, 0, OK, OK, 0, -1000},
        {{"-tvstd", "secam"}, 0, FLAG, FLAG, 0, -1000},
        {{"-tvstd"}, 0, FLAG, FLAG, 0, -1000},
        {{"-width", "31"}, 0, FLAG, FLAG, 0, -1000},
        {{"-width", "0x40"}, 0, OK, OK, 0, -1000},
        {{"-width"}, 0, FLAG, FLAG, 0, -1000},
        {{"-i"}, 0, FLAG, FLAG, 0, -1000},
        {{"-o"}, 0, FLAG, FLAG, 0, -1000},
        {{"-h"}, 0, HELP, HELP, 0, -1000},
        {{"-i", "a", "--help", "-bogus"}, 0, HELP, HELP, 0, -1000},
        {{"-bogus"}, 0, FLAG, FLAG, 0, -1000},
        {{"stray"}, 0, FLAG, FLAG, 0, -1000},
        {{"-422", "-420", "---422"}, 0, OK, OK, 0, -1000},
    };
    for (size_t index = 0; index < cases.size(); index++) {
        const Case &c = cases[index];
        // argv as main() gets it: exactly argc + 1 pointers, the last NULL, in a block of its own so that a read
        // behind it is seen
        std::vector<const char *> argv;
        argv.push_back("tool");
        argv.insert(argv.end(), c.flags.begin(), c.flags.end());
        argv.push_back(nullptr);
        argv.shrink_to_fit();
        const int argc = (int)argv.size() - 1;
        for (int stage = 0; stage < 2; stage++) {
            ntscsim_pixmap_params p;
            if (stage == 0) ntscsim_post_params_init(&p);
            else ntscsim_cmap_params_init(&p);
            const int rc = stage == 0 ? ntscsim_post_parse_argv(&p, argc, argv.data(), c.require_io)
                                      : ntscsim_cmap_parse_argv(&p, argc, argv.data(), c.require_io);
            expect(rc == (stage == 0 ? c.post : c.cmap), stage == 0 ? "posterize return code" : "colormap return code", index);
            if (rc == NTSCSIM_OK) {
                expect(p.n_layers == c.n_layers && p.n_layers <= p.layers_cap, "n_layers", index);
                for (int l = 0; l < p.n_layers; l++) expect(p.layers[l].path && std::strlen(p.layers[l].path) == 1, "path", index);
                if (stage == 0 && c.last_threshhold != -1000)
                    expect(p.n_layers > 0 && p.layers[p.n_layers - 1].threshhold == c.last_threshhold, "threshhold", index);
                if (stage == 1)
                    for (int l = 0; l < p.n_layers; l++) expect(p.layers[l].threshhold == 3, "colormap threshhold", index);
            }
            // a failed parse leaves the inputs it had opened: free releases them either way, and twice is harmless
            if (stage == 0) ntscsim_post_params_free(&p);
            else ntscsim_cmap_params_free(&p);
            expect(p.layers == nullptr && p.n_layers == 0 && p.layers_cap == 0, "free", index);
            ntscsim_pixmap_params_free(&p);
        }
    }
    ntscsim_pixmap_params_free(nullptr);
    std::printf("%zu argument vectors through both parsers, %d bad\n", cases.size(), bad);
    return bad ? 1 : 0;
}
