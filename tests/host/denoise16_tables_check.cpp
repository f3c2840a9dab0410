// denoise16_tables_check.cpp -- the 16-bit denoise stage's host-built tables (csrc/uva_denoise16_tables.h) in a program of
// their own: no HIP, no GPU.  Writes every integer to the file named on the command line, as little-endian int64:
//   ftab[65536], fwd[9], inv[9], l_mul, l_sub, a_mul, b_mul, il_mul, il_add, ia_mul, ib_mul, f_thr, f_bias, lin_mul,
//   then for each (h, cn) argument pair: n, table[n].
// tests/test_denoise16.py compares them with the numpy definition's.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../upscale_video_amd/csrc/uva_denoise16_tables.h"

static void put(FILE* f, int64_t v) { std::fwrite(&v, sizeof v, 1, f); }

int main(int argc, char** argv)
{
    if (argc < 2 || (argc - 2) % 2) {
        std::fprintf(stderr, "usage: denoise16_tables_check OUT [h cn]...\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    auto t = std::make_unique<uva::Lab16Tables>();
    uva::lab16_tables_host(*t);
    for (uint32_t v : t->ftab) put(f, v);
    for (uint32_t v : t->fwd) put(f, v);
    for (int64_t v : t->inv) put(f, v);
    for (int64_t v : {t->l_mul, t->l_sub, t->a_mul, t->b_mul, t->il_mul, t->il_add, t->ia_mul, t->ib_mul, t->f_thr, t->f_bias, t->lin_mul})
        put(f, v);
    for (int i = 2; i + 1 < argc; i += 2) {
        std::vector<int> tab;
        if (!uva::nlm16_weight_table((float)std::atof(argv[i]), std::atoi(argv[i + 1]), tab)) return 3;
        put(f, (int64_t)tab.size());
        for (int v : tab) put(f, v);
    }
    if (std::fclose(f)) return 2;
    std::printf("denoise16_tables_check: %d weight tables: ok\n", (argc - 2) / 2);
    return 0;
}
