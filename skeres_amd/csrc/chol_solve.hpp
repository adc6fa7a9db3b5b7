// sk_cholesky_solve* behind their argument checks (chol_solve.hip): the fronts of chol_fronts.hpp on the device.  SK_* status;
// the message of a failure is set.
#pragma once

namespace sk {

// one front; last: a caller's block envelope or nullptr; border_begin_row >= 0: the bordered envelope of the matrix itself
int cholesky_solve_single(int n, const double* A, const double* b, double* x, double* L, int group, const int* last, int automatic_plan, int border_begin_row);
int cholesky_solve_two_way(int n, const double* A, const double* b, double* x, int head, int tail_begin, int group, int automatic_plan);
int cholesky_solve_multi_way(int n, const double* A, const double* b, double* x, int num_segments, const int* cuts, int group, int automatic_plan);

}  // namespace sk
