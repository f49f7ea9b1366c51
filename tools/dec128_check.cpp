// dec128_check: host build of galaxysql_amd/csrc/gx_dec128.h, the 128-bit
// helpers behind GX_AGG_SUM_DEC / GX_AGG_AVG_DEC, driven line by line from
// stdin so a test can compare them with big-integer arithmetic:
//   D <hex80> <scale>            -> fence neg hi lo      (gx_dec40_to_u128)
//   E <hi> <lo> <neg> <scale>    -> hex80                (gx_u128_to_dec40)
//   A <hi> <lo> <count> <scale>  -> hi lo                (gx_dec_avg4)
//   Q <hi> <lo> <d>              -> qhi qlo rem          (gx_u128_divmod_u64)
// Numbers are decimal u64. Build: g++ -O1 -I galaxysql_amd/csrc.
#include <cstdio>
#include <cstring>
#include <string>

#include "gx_dec128.h"

int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'D') {
            char hex[128];
            int scale;
            if (scanf("%100s %d", hex, &scale) != 2 || strlen(hex) != 80)
                return 2;
            alignas(8) uint8_t p[40];
            for (int i = 0; i < 40; i++) {
                unsigned b;
                sscanf(hex + 2 * i, "%2x", &b);
                p[i] = (uint8_t)b;
            }
            gx_u128 mag = {0, 0};
            bool neg = false;
            uint32_t f = gx_dec40_to_u128(p, scale, &mag, &neg);
            if (f) mag.lo = mag.hi = 0;
            printf("%u %d %llu %llu\n", f, (int)neg, mag.hi, mag.lo);
        } else if (op == 'E') {
            gx_u128 m;
            int neg, scale;
            if (scanf("%llu %llu %d %d", &m.hi, &m.lo, &neg, &scale) != 4)
                return 2;
            alignas(8) uint8_t p[40];
            gx_u128_to_dec40(m, neg != 0, scale, p);
            for (int i = 0; i < 40; i++) printf("%02x", p[i]);
            printf("\n");
        } else if (op == 'A') {
            gx_u128 m;
            unsigned long long count;
            int scale;
            if (scanf("%llu %llu %llu %d", &m.hi, &m.lo, &count, &scale) != 4)
                return 2;
            gx_u128 r = gx_dec_avg4(m, count, scale);
            printf("%llu %llu\n", r.hi, r.lo);
        } else if (op == 'Q') {
            gx_u128 m;
            unsigned long long d;
            if (scanf("%llu %llu %llu", &m.hi, &m.lo, &d) != 3) return 2;
            unsigned long long rem = gx_u128_divmod_u64(m, d);
            printf("%llu %llu %llu\n", m.hi, m.lo, rem);
        } else {
            return 2;
        }
    }
    return 0;
}
