// Stand-alone check of the launch shapes of the wave-per-codeword decoders (wave_cw_plan.h and
// the families' *_layout.h) against tests/golden/wave_cw_choices.json, the table recorded from
// the *_choose functions before they shared a planner. Built with -fsanitize=address,undefined
// by tests/test_wave_cw.py; usage: wave_cw_host <table.json>.
#include "fxlms_layout.h"
#include "fxms_layout.h"
#include "hwgdbf_layout.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

using Row = std::map<std::string, std::string>;

// The table is a JSON list of flat objects whose values are strings or integers.
static std::vector<Row> read_table(const std::string &text)
{
    std::vector<Row> rows;
    size_t i = 0;
    auto str = [&]() {   // at an opening quote
        const size_t e = text.find('"', i + 1);
        if (e == std::string::npos) throw std::runtime_error("unterminated string");
        const std::string s = text.substr(i + 1, e - i - 1);
        i = e + 1;
        return s;
    };
    while ((i = text.find('{', i)) != std::string::npos) {
        Row r;
        const size_t end = text.find('}', i);
        if (end == std::string::npos) throw std::runtime_error("unterminated object");
        while ((i = text.find('"', i)) != std::string::npos && i < end) {
            const std::string key = str();
            i = text.find(':', i) + 1;
            while (text[i] == ' ') ++i;
            if (text[i] == '"') {
                r[key] = str();
            } else {
                const size_t e = text.find_first_of(",}", i);
                r[key] = text.substr(i, e - i);
                i = e;
            }
        }
        i = end + 1;
        rows.push_back(r);
    }
    return rows;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::vector<Row> rows = read_table(ss.str());
    int failures = 0, named = 0;
    for (const Row &r : rows) {
        auto num = [&](const char *k) { return std::atoi(r.at(k).c_str()); };
        const std::string fam = r.at("family");
        const ldpc::WaveCwSizes z{num("N"), num("M"), num("dcs"), num("E")};
        ldpc::WaveCwChoice ch;
        int wave = 1;
        if (fam == "fxms") {
            ch = ldpc::fxms_plan(z, num("arg"));
        } else if (fam == "fxlms") {
            ch = ldpc::fxlms_plan(z, num("arg"));
        } else if (fam == "hwgdbf") {
            const ldpc::HwgdbfChoice h = ldpc::hwgdbf_plan(z, num("arg"), num("opt") == 1);
            ch = h;
            wave = h.wave;
        } else {
            std::printf("unknown family %s\n", fam.c_str());
            return 2;
        }
        if (!ch.name[0]) wave = 0;
        named += ch.name[0] != 0;
        const bool ok = r.at("name") == ch.name && num("threads") == ch.threads && num("cw_per_block") == ch.cw_per_block &&
                        num("lds_bytes") == ch.lds_bytes && num("cw_bytes") == ch.cw_bytes && num("staged") == (int)ch.staged &&
                        num("wave") == wave;
        if (!ok) {
            ++failures;
            std::printf("MISMATCH %s N %d M %d dcs %d E %d arg %d opt %d (%s): got '%s' threads %d cw_per_block %d lds %d cw %d "
                        "staged %d wave %d\n",
                        fam.c_str(), z.N, z.M, z.dcs, z.E, num("arg"), num("opt"), r.at("note").c_str(), ch.name, ch.threads,
                        ch.cw_per_block, ch.lds_bytes, ch.cw_bytes, (int)ch.staged, wave);
        }
    }
    // where not even one codeword fits beside the graph the planner says so, whichever way a tie goes
    for (bool tie : {false, true}) {
        const ldpc::WaveCwPlan p = ldpc::wave_cw_plan(ldpc::kWaveCwLds - 1000, 1000, 32, tie);
        if (p.waves != 0 || p.cw_per_block != 0) {
            ++failures;
            std::printf("MISMATCH nothing fits: waves %d cw_per_block %d\n", p.waves, p.cw_per_block);
        }
    }
    if (ldpc::wave_cw_waves(0, 65536, 1, 4, 24) != 8 || ldpc::wave_cw_waves(98304, 65536, 1, 4, 24) != 0) {
        ++failures;
        std::printf("MISMATCH wave_cw_waves\n");
    }
    std::printf("%zu rows, %d with a kernel: %s (%d failures)\n", rows.size(), named, failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
