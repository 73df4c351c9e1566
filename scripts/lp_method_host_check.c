/* Stand-alone check of the host-only paths of the LP method options, for a run under -fsanitize=address,undefined (no GPU, no Python):
 *   - the flag helpers of include/bslv_hip.h: BSLV_VLP_LP_METHOD / BSLV_VLP_LP_METHOD_OF round-trip for every phase and method, leave
 *     the four older flags alone, and decode "nothing given" as -1;
 *   - the mapping of lp_set_options (bslv_lp_compat_method, host/bslv_lp_compat.c) over every phase_type x lp_method_type, against the
 *     table of the reference's lp_set_options written out below, the values outside the enums included.
 * cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -o /tmp/lp_method_host_check scripts/lp_method_host_check.c \
 *    bensolve_amd/csrc/host/bslv_lp_compat.c -Lbensolve_amd/csrc -lbslv_hip -Wl,-rpath,$PWD/bensolve_amd/csrc -lm && /tmp/lp_method_host_check */
#include <stdio.h>
#include <stdlib.h>
#include "../include/bslv_hip.h"
#include "../include/bslv_lp_compat.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main(void)
{
    const int old = BSLV_VLP_PHASE1_DUAL | BSLV_VLP_PREIMAGES | BSLV_VLP_CANONICAL | BSLV_VLP_CANONICAL_CALL;
    for (int a = -1; a <= 2; a++) for (int b = -1; b <= 2; b++) for (int c = -1; c <= 2; c++) {
        int flags = old;
        if (a >= 0) flags |= BSLV_VLP_LP_METHOD(0, a);
        if (b >= 0) flags |= BSLV_VLP_LP_METHOD(1, b);
        if (c >= 0) flags |= BSLV_VLP_LP_METHOD(2, c);
        CHECK(BSLV_VLP_LP_METHOD_OF(flags, 0) == a && BSLV_VLP_LP_METHOD_OF(flags, 1) == b && BSLV_VLP_LP_METHOD_OF(flags, 2) == c);
        CHECK((flags & 15) == old && (flags >> 10) == 0);
    }
    CHECK(BSLV_VLP_LP_METHOD_OF(old, 0) == -1 && BSLV_VLP_LP_METHOD_OF(0, 2) == -1);
    /* rows: PHASE0, PHASE1_PRIMAL, PHASE1_DUAL, PHASE2_PRIMAL, PHASE2_DUAL; -9 = "prev" */
    static const int own[5] = {-9, BSLV_LP_METHOD_DUAL, BSLV_LP_METHOD_PRIMAL, BSLV_LP_METHOD_DUAL, BSLV_LP_METHOD_PRIMAL};
    static const int given[3] = {BSLV_LP_METHOD_PRIMAL, BSLV_LP_METHOD_DUAL, BSLV_LP_METHOD_REPAIR};
    for (int ph = 0; ph < 5; ph++) for (int m = 0; m < 4; m++) for (int prev = 0; prev < 3; prev++) {
        struct lp_opt o = {LP_METHOD_AUTO, LP_METHOD_AUTO, LP_METHOD_AUTO, 0};
        /* the option of the phase at hand is m; the two others hold something else, which must not be read */
        o.method_phase0 = ph == 0 ? (lp_method_type)m : DUAL_PRIMAL_SIMPLEX;
        o.method_phase1 = (ph == 1 || ph == 2) ? (lp_method_type)m : PRIMAL_SIMPLEX;
        o.method_phase2 = (ph == 3 || ph == 4) ? (lp_method_type)m : DUAL_SIMPLEX;
        const int want = m == (int)LP_METHOD_AUTO ? (own[ph] == -9 ? prev : own[ph]) : given[m];
        CHECK(bslv_lp_compat_method(&o, (phase_type)ph, prev) == want);
    }
    {
        struct lp_opt o = {LP_METHOD_AUTO, LP_METHOD_AUTO, LP_METHOD_AUTO, 0};
        CHECK(bslv_lp_compat_method(NULL, PHASE0, 0) == -1);
        CHECK(bslv_lp_compat_method(&o, (phase_type)5, 0) == -1 && bslv_lp_compat_method(&o, (phase_type)-1, 0) == -1);
        o.method_phase1 = (lp_method_type)4;
        CHECK(bslv_lp_compat_method(&o, PHASE1_DUAL, 0) == -1);
        o.method_phase1 = (lp_method_type)-1;
        CHECK(bslv_lp_compat_method(&o, PHASE1_PRIMAL, 0) == -1);
    }
    printf(fails ? "lp_method_host_check: %d FAILED\n" : "lp_method_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
