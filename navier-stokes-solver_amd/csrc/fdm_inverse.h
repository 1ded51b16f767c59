// What the fused loops see of the fast-diagonalisation inverse (fdm_inverse.hip): its rows and its apply.
#pragma once

#include "nss_common.h"

struct nss_fdmi_s;

namespace nss {

int64_t fdmi_rows(const nss_fdmi_s& h);                    // n_total of the vector it was made for

// y = scale * A^-1 x on the components (x != y; every other entry of y keeps its bits): 2 dim launches on `st`, each of
// which returns at once when `done` (device int, may be NULL) is non-zero
void fdmi_apply(const nss_fdmi_s& h, double scale, const double* x, double* y, const int32_t* done, hipStream_t st);

}  // namespace nss
