// enc_group_host.cc -- pomegranate_amd/csrc/lzo1x_enc_group.h on the CPU
// (never part of the product library).
//   libenc_group_host.so  enc_group_*_host(): the header's functions one by
//                         one; enc_group_walk_host(): every (workgroup, wave)
//                         of a launch walked as the kernel walks them, with
//                         what tests/test_enc_group.py asserts counted up
//   enc_group_check       (-DENC_GROUP_CHECK) the same walk for every grid
//                         0..70 and the shapes 4+1, 8+1 and 8+2, the owner
//                         counts in heap arrays of exactly their size
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "lzo1x_enc_group.h"

extern "C" {

struct enc_group_walk {
    uint32_t workgroups;        // enc_group_workgroups
    uint32_t owned;             // regions with exactly one owner
    uint32_t multi;             // regions with more than one owner
    uint32_t past;              // live parse waves whose region is not below the grid
    uint32_t idle;              // idle parse waves
    uint32_t idle_outside_last; // idle parse waves in a workgroup other than the last
    uint32_t slots_served;      // parse slots of a workgroup with exactly one emit wave
    uint32_t slots_unserved;    // parse slots of a workgroup with none, or more than one
};

uint32_t enc_group_workgroups_host(uint32_t regions, uint32_t group) { return enc_group_workgroups(regions, group); }
uint32_t enc_group_region_host(uint32_t wg, uint32_t wave, uint32_t group) { return enc_group_region(wg, wave, group); }
int enc_group_idle_host(uint32_t wg, uint32_t wave, uint32_t group, uint32_t regions)
{
    return enc_group_idle(wg, wave, group, regions);
}
int enc_group_use_host(uint32_t regions, uint32_t group, uint32_t cus) { return enc_group_use(regions, group, cus); }

int enc_group_walk_host(uint32_t regions, uint32_t group, uint32_t emitters, enc_group_walk* r)
{
    *r = enc_group_walk();
    r->workgroups = enc_group_workgroups(regions, group);
    uint32_t* owners = (uint32_t*)calloc(regions ? regions : 1, sizeof(uint32_t));
    uint32_t* served = (uint32_t*)calloc(group, sizeof(uint32_t));
    if (!owners || !served)
        return -1;
    for (uint32_t wg = 0; wg < r->workgroups; wg++)
        for (uint32_t w = 0; w < group; w++) {
            if (enc_group_idle(wg, w, group, regions)) {
                r->idle++;
                r->idle_outside_last += wg + 1 != r->workgroups;
                continue;
            }
            const uint32_t reg = enc_group_region(wg, w, group);
            if (reg >= regions)
                r->past++;
            else
                owners[reg]++;                       // (ASan: exactly `regions` entries)
        }
    for (uint32_t i = 0; i < regions; i++) {
        r->owned += owners[i] == 1;
        r->multi += owners[i] > 1;
    }
    for (uint32_t e = 0; e < emitters; e++) {
        const uint32_t s0 = enc_group_emit_first(e, group, emitters);
        for (uint32_t s = s0; s < s0 + enc_group_emit_count(e, group, emitters); s++)
            served[s]++;                             // (ASan: exactly `group` entries)
    }
    for (uint32_t s = 0; s < group; s++) {
        r->slots_served += served[s] == 1;
        r->slots_unserved += served[s] != 1;
    }
    free(owners);
    free(served);
    return 0;
}

}  // extern "C"

#ifdef ENC_GROUP_CHECK
int main()
{
    static const uint32_t shapes[3][2] = {{4, 1}, {8, 1}, {8, 2}};
    unsigned bad = 0;
    for (const auto& sh : shapes)
        for (uint32_t grid = 0; grid <= 70; grid++) {
            enc_group_walk r;
            if (enc_group_walk_host(grid, sh[0], sh[1], &r) != 0)
                return 2;
            const uint32_t ceil_wg = (grid + sh[0] - 1) / sh[0];
            const bool ok = r.workgroups == ceil_wg && r.owned == grid && r.multi == 0 && r.past == 0 &&
                            r.idle == ceil_wg * sh[0] - grid && r.idle_outside_last == 0 &&
                            r.slots_served == sh[0] && r.slots_unserved == 0;
            if (!ok) {
                printf("enc_group_check: grid %u shape %u+%u wrong\n", grid, sh[0], sh[1]);
                bad++;
            }
        }
    // the selection rule at its edges (256 CUs, groups of 4)
    bad += enc_group_use(0, 4, 256) || enc_group_use(3, 4, 256) || enc_group_use(4, 4, 256);
    bad += enc_group_use(1020, 4, 256) || !enc_group_use(1021, 4, 256) || !enc_group_use(4096, 4, 256);
    bad += !enc_group_use(4, 4, 1) || enc_group_use(3, 4, 1);
    if (bad)
        return 1;
    printf("enc_group_check: ok\n");
    return 0;
}
#endif
