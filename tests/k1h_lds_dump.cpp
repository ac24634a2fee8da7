// Host program of tests/test_k1h_lds_host.py: evaluates the LDS address
// functions of K1h's 16x16x32 form (confild_amd/csrc/k1h_lds.hpp) for every lane
// of every ds_read_b128 and staging store the kernel issues, with the kernel's
// thread roles (conv_x.hip, conv_h16_body), and prints one line per wave
// instruction: a tag, its parameters, then 64 byte addresses (-1: lane inactive).
//   A swz tw phase wm ty tx i | addresses in one halo plane
//   B swz bn wn j             | addresses in one ring plane
//   S swz tw bn it wave       | 8-byte halo staging stores
//   W swz bn wave             | 16-byte weight staging stores
#include <cstdio>
#include <initializer_list>

#include "k1h_lds.hpp"

using namespace cfd;

int main() {
    const int BM = 256;
    for (int swz = 1; swz >= 0; --swz) {
        for (int tw : {64, 32, 16}) {
            for (int phase = 0; phase < 2; ++phase)
                for (int wm = 0; wm < BM / 64; ++wm)
                    for (int ty = 0; ty < (phase ? 2 : 3); ++ty)
                        for (int tx = 0; tx < (phase ? 2 : 3); ++tx)
                            for (int i = 0; i < 4; ++i) {
                                printf("A %d %d %d %d %d %d %d", swz, tw, phase, wm, ty, tx, i);
                                for (int lane = 0; lane < 64; ++lane)
                                    printf(" %d", k1h_a_base(tw, wm, lane & 15, lane >> 4, tx, swz) + k1h_a_imm(tw, i, ty));
                                printf("\n");
                            }
            for (int bn : {128, 64}) {
                const int ntg = 64 * (BM / 64) * (bn / 64);
                const int npxd = k1h_npx_staged(BM, tw);
                const int hit = (npxd * 8 + ntg - 1) / ntg;
                for (int it = 0; it < hit; ++it)
                    for (int wave = 0; wave < ntg / 64; ++wave) {
                        printf("S %d %d %d %d %d", swz, tw, bn, it, wave);
                        for (int lane = 0; lane < 64; ++lane) {
                            const int gt = wave * 64 + lane, e = gt + it * ntg;
                            printf(" %d", e < npxd * 8 ? k1h_stage_off(tw, e >> 3, gt & 7, swz) : -1);
                        }
                        printf("\n");
                    }
            }
        }
        for (int bn : {128, 64}) {
            for (int wn = 0; wn < bn / 64; ++wn)
                for (int j = 0; j < 4; ++j) {
                    printf("B %d %d %d %d", swz, bn, wn, j);
                    for (int lane = 0; lane < 64; ++lane) printf(" %d", k1h_b_base(wn, lane & 15, lane >> 4, swz) + k1h_b_imm(j));
                    printf("\n");
                }
            const int ntg = 64 * (BM / 64) * (bn / 64);
            for (int wave = 0; wave < ntg / 64; ++wave) {
                printf("W %d %d %d", swz, bn, wave);
                for (int lane = 0; lane < 64; ++lane) {
                    const int gt = wave * 64 + lane;
                    printf(" %d", k1h_wstage_off(gt >> 2, gt & 3, swz));
                }
                printf("\n");
            }
        }
    }
    return 0;
}
