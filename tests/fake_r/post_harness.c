/* tests/fake_r/post_harness.c -- plays R's part of `.Call("_topolow_post_metrics", positions, values, codes, want_est)`
 * on the test double of R's C API: fake_r.c is taken in whole (its own main renamed away), so the double stays as it is.
 *   post_harness <input file>
 * The input file is text: "n ndim vn cn want_est", then positions (n x ndim), values (vn x vn; "Inf", "-inf", "nan"
 * allowed) and, if cn > 0, codes (cn x cn; cn = 0: NULL), all column-major.  vn != n or cn != n makes the call a bad one.
 * The result list (or the R error) is printed as one JSON object.  Test infrastructure only
 * (tests/test_post_metrics_capi.py, tests/test_gpu_post_metrics.py). */
#define main fake_r_call_harness_main
#include "fake_r.c"
#undef main

static void print_real(double x) {
  if (isnan(x)) printf("NaN");
  else if (isinf(x)) printf(x > 0 ? "Infinity" : "-Infinity");
  else printf("%.17g", x);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  R_init_topolow(&dll);
  typedef SEXP (*call4)(SEXP, SEXP, SEXP, SEXP);
  call4 fn = (call4)find_routine("_topolow_post_metrics", 4);
  if (!fn || dll.use_dynamic_symbols != FALSE) { printf("{\"registration\": \"bad\"}\n"); return 1; }
  const int n = (int)read_num(f), ndim = (int)read_num(f), vn = (int)read_num(f);
  const int cn = (int)read_num(f), want_est = (int)read_num(f);
  SEXP pos = read_real(f, n, ndim), values = read_real(f, vn, vn);
  SEXP codes = cn > 0 ? read_int(f, cn, cn) : R_NilValue;
  fclose(f);
  if (setjmp(error_jmp) != 0) {
    printf("{\"registration\": \"ok\", \"error\": ");
    print_json_string(error_msg);
    printf(", \"protect_depth\": %d}\n", protect_depth);
    return 0;
  }
  SEXP out = fn(pos, values, codes, Rf_ScalarLogical(want_est));
  SEXP names = Rf_getAttrib(out, R_NamesSymbol);
  printf("{\"registration\": \"ok\", \"error\": null, \"names\": [");
  for (int i = 0; i < Rf_length(names); ++i) printf("%s\"%s\"", i ? ", " : "", CHAR(STRING_ELT(names, i)));
  SEXP est = VECTOR_ELT(out, 0);
  printf("], \"est_distances\": ");
  if (est == R_NilValue) {
    printf("null, \"est_dim\": null");
  } else {
    printf("[");
    for (R_xlen_t i = 0; i < XLENGTH(est); ++i) { if (i) printf(", "); print_real(REAL(est)[i]); }
    printf("], \"est_dim\": [%d, %d]", Rf_nrows(est), Rf_ncols(est));
  }
  printf(", \"mae\": ");
  print_real(REAL(VECTOR_ELT(out, 1))[0]);
  printf(", \"sum_abs\": ");
  print_real(REAL(VECTOR_ELT(out, 2))[0]);
  printf(", \"count\": ");
  print_real(REAL(VECTOR_ELT(out, 3))[0]);
  printf(", \"protect_depth\": %d}\n", protect_depth);
  return 0;
}
