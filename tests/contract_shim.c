/* contract_shim.c — the binary64 functions of include/ptmi_math.h behind a C ABI, for
 * tests/test_numerics_contract.py::test_sets_tell_a_contracted_build, which compiles this file twice: with the oracle's flags
 * and with -mfma -ffp-contract=fast.  Same op numbers as PTMI_MATH_*_D (include/ptmi.h). */
#include "../include/ptmi_math.h"

void shim_math_d(int op, int n, const float* a, const float* b, double* out /* n*2 */) {
    for (int i = 0; i < n; i++) {
        double r0 = 0.0, r1 = 0.0;
        switch (op) {
            case 0: ptmi_sincos_d((double)a[i], &r0, &r1); break;
            case 1: r0 = ptmi_tan_d((double)a[i]); break;
            case 2: r0 = ptmi_log_d((double)a[i]); break;
            case 3: r0 = ptmi_exp_d((double)a[i]); break;
            case 4: r0 = ptmi_atan2_d((double)a[i], (double)b[i]); break;
            default: break;
        }
        out[2 * i] = r0; out[2 * i + 1] = r1;
    }
}
