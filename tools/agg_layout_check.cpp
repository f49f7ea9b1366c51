// agg_layout_check: host build of galaxysql_amd/csrc/gx_agg_layout.h, the one
// definition of the aggregate state record, driven line by line from stdin so
// a test can compare it with the rule written out independently:
//   L f0 f1 ...          -> stride | val_off.. | seen_off.. | tmpl words (hex)
//                           | tmpl_zero | result types
//   S f0 f1 ... | i j .. -> n_aggs stride | func.. | val_off.. | seen_off..
//                           of AggLayout::select
//   V func val seen      -> bits (hex) isnull   (agg_decode of record
//                           {val, seen}; a func without a seen slot ignores
//                           `seen`)
// Funcs are base gx_agg_func numbers; val / seen are hex u64.
// Build: g++ -O1 -std=c++17 -I galaxysql_amd/csrc -I include.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "gx_agg_layout.h"

static void print_ints(const int32_t *v, int n) {
    printf(" |");
    for (int i = 0; i < n; i++) printf(" %d", v[i]);
}

int main() {
    char buf[4096];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        char op;
        if (!(in >> op)) continue;
        if (op == 'L' || op == 'S') {
            std::vector<int32_t> funcs, idx;
            std::string tok;
            bool after_bar = false;
            while (in >> tok) {
                if (tok == "|") { after_bar = true; continue; }
                (after_bar ? idx : funcs).push_back((int32_t)std::stol(tok));
            }
            if (funcs.size() > GX_MAX_COLS || idx.size() > GX_MAX_COLS)
                return 2;
            for (int32_t i : idx)
                if (i < 0 || (size_t)i >= funcs.size()) return 2;
            AggLayout L;
            L.build(funcs.data(), (int)funcs.size());
            if (op == 'L') {
                const AggRecDesc &R = L.desc;
                if (R.stride > 3 * GX_MAX_COLS) return 3;
                printf("%d", R.stride);
                print_ints(R.val_off, R.n_aggs);
                print_ints(R.seen_off, R.n_aggs);
                printf(" |");
                for (int k = 0; k < R.stride; k++) printf(" %llx", L.tmpl[k]);
                printf(" | %d", (int)L.tmpl_zero);
                printf(" |");
                for (int a = 0; a < R.n_aggs; a++)
                    printf(" %d", agg_func_result_type(R.func[a]));
                printf("\n");
            } else {
                const AggRecDesc d = L.select(idx.data(), (int)idx.size());
                printf("%d %d", d.n_aggs, d.stride);
                print_ints(d.func, d.n_aggs);
                print_ints(d.val_off, d.n_aggs);
                print_ints(d.seen_off, d.n_aggs);
                printf("\n");
            }
        } else if (op == 'V') {
            int32_t func;
            unsigned long long rec[2];
            if (!(in >> func >> std::hex >> rec[0] >> rec[1])) return 2;
            const AggDecoded d = agg_decode(
                func, rec, 0, agg_func_tracks_null(func) ? 1 : -1);
            printf("%llx %d\n", d.bits, (int)d.isnull);
        } else {
            return 2;
        }
    }
    return 0;
}
