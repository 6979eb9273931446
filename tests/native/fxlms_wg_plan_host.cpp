// Stand-alone driver of the host-only launch planners (fxlms_layout.h and the headers it
// shares with fxms and hwgdbf): answers queries read from a file, one a line,
//   <family> N M dcs E arg opt      family: fxms | fxlms | hwgdbf | fxlms_wg
// with one line each,
//   <name or -> threads cw_per_block lds_bytes cw_bytes staged wave wg slot_bytes s1off mgoff hi
// (arg: msg_bits, app_bits or qlen; opt: option gdbf_kernel; the last five are fxlms_wg's and 0
// elsewhere). tests/test_fxlms_wg_host.py builds it with -fsanitize=address,undefined, asks
// for the recorded table tests/golden/wave_cw_choices.json and for fxlms_wg_plan on the test
// codes and on sizes at the LDS bound, and compares.
#include "fxlms_layout.h"
#include "fxms_layout.h"
#include "hwgdbf_layout.h"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string fam;
        ldpc::WaveCwSizes z{};
        int arg = 0, opt = 0;
        if (!(in >> fam >> z.N >> z.M >> z.dcs >> z.E >> arg >> opt)) return 2;
        ldpc::FxlmsChoice ch;
        ldpc::FxlmsWgLayout L{};
        int wave = 1;
        if (fam == "fxms") {
            static_cast<ldpc::FxmsChoice &>(ch) = ldpc::fxms_plan(z, arg);
        } else if (fam == "fxlms") {
            ch = ldpc::fxlms_plan(z, arg);
        } else if (fam == "hwgdbf") {
            const ldpc::HwgdbfChoice h = ldpc::hwgdbf_plan(z, arg, opt == 1);
            static_cast<ldpc::WaveCwChoice &>(ch) = h;
            wave = h.wave;
        } else if (fam == "fxlms_wg") {
            ch = ldpc::fxlms_wg_plan(z, arg);
            L = ldpc::fxlms_wg_layout(z, ch.wide);
            wave = 0;
        } else {
            return 2;
        }
        if (!ch.name[0]) wave = 0;
        std::printf("%s %d %d %d %d %d %d %d %d %d %d %d\n", ch.name[0] ? ch.name : "-", ch.threads, ch.cw_per_block, ch.lds_bytes,
                    ch.cw_bytes, (int)ch.staged, wave, (int)ch.wg, ch.slot_bytes, ch.wg ? L.s1off : 0, ch.wg ? L.mgoff : 0,
                    ch.wg ? L.hi : 0);
    }
    return 0;
}
