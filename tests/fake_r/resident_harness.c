/* tests/fake_r/resident_harness.c -- plays R's part of
 *   .Call("_topolow_euclidean_embedding_resident", values, codes, order, initial_positions, ndim, mapping_max_iter, k0,
 *         cooling_rate, c_repulsion, relative_epsilon, convergence_counter, convergence_check_freq, preserve_order,
 *         verbose, want_est)
 * on the test double of R's C API: fake_r.c is taken in whole (its own main renamed away), so the double stays as it is.
 *   resident_harness <input file>
 * The input file is text:
 *   "n ndim vn cn on pr pc want_est preserve_order verbose n_iter window check_freq seed interrupt_after bad"
 *   "k0 cooling_rate c_repulsion relative_epsilon"
 * then values (vn x vn; "nan", "inf", "-inf" allowed), codes (cn x cn; cn = 0: NULL), order (on entries, 1-based;
 * on = 0: NULL) and initial_positions (pr x pc), all column-major.  `bad` makes the call a badly typed one: 1 values
 * as an integer matrix, 2 codes as a numeric matrix, 3 order as a numeric vector, 4 initial_positions as an integer
 * matrix, 5 values as a plain vector; sizes that disagree (vn, cn, on, pr, pc against n, ndim) do the same.  seed >= 0
 * sets options(topolow.seed); interrupt_after > 0 makes R's interrupt check fire at that poll.
 * The result list (or the R error) is printed as one JSON object.  Test infrastructure only
 * (tests/test_resident_embedding_capi.py, tests/test_gpu_resident_embedding.py). */
#define main fake_r_call_harness_main
#include "fake_r.c"
#undef main

static void print_real(double x) {
  if (isnan(x)) printf("NaN");
  else if (isinf(x)) printf(x > 0 ? "Infinity" : "-Infinity");
  else printf("%.17g", x);
}

static void print_reals(SEXP v) {
  if (v == R_NilValue) { printf("null"); return; }
  printf("[");
  for (R_xlen_t i = 0; i < XLENGTH(v); ++i) { if (i) printf(", "); print_real(REAL(v)[i]); }
  printf("]");
}

static void print_scalar(SEXP v) {
  if (v == R_NilValue) printf("null");
  else if (v->type == REALSXP) print_real(REAL(v)[0]);
  else printf("%d", INTEGER(v)[0]);
}

static SEXP as_int_matrix(SEXP x) {
  SEXP y = Rf_allocMatrix(INTSXP, Rf_nrows(x), Rf_ncols(x));
  for (R_xlen_t i = 0; i < XLENGTH(x); ++i) INTEGER(y)[i] = isfinite(REAL(x)[i]) ? (int)REAL(x)[i] : 0;
  return y;
}

static SEXP as_real(SEXP x, int matrix) {
  SEXP y = matrix ? Rf_allocMatrix(REALSXP, Rf_nrows(x), Rf_ncols(x)) : Rf_allocVector(REALSXP, XLENGTH(x));
  for (R_xlen_t i = 0; i < XLENGTH(x); ++i) REAL(y)[i] = (double)INTEGER(x)[i];
  return y;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  R_init_topolow(&dll);
  typedef SEXP (*call15)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
  call15 fn = (call15)find_routine("_topolow_euclidean_embedding_resident", 15);
  if (!fn || dll.use_dynamic_symbols != FALSE) { printf("{\"registration\": \"bad\"}\n"); return 1; }
  const int n = (int)read_num(f), ndim = (int)read_num(f), vn = (int)read_num(f), cn = (int)read_num(f);
  const int on = (int)read_num(f), pr = (int)read_num(f), pc = (int)read_num(f), want_est = (int)read_num(f);
  const int preserve = (int)read_num(f), verbose = (int)read_num(f), n_iter = (int)read_num(f);
  const int window = (int)read_num(f), freq = (int)read_num(f);
  const double seed = read_num(f);
  fake_r_interrupt_after = (int)read_num(f);
  const int bad = (int)read_num(f);
  const double k0 = read_num(f), cooling = read_num(f), c_rep = read_num(f), eps = read_num(f);
  (void)n;
  SEXP values = read_real(f, vn, vn);
  SEXP codes = cn > 0 ? read_int(f, cn, cn) : R_NilValue;
  SEXP order = on > 0 ? read_int(f, on, 0) : R_NilValue;
  SEXP init = read_real(f, pr, pc);
  fclose(f);
  if (seed >= 0.0) fake_r_set_option_real("topolow.seed", seed);
  if (bad == 1) values = as_int_matrix(values);
  if (bad == 2 && codes != R_NilValue) codes = as_real(codes, 1);
  if (bad == 3 && order != R_NilValue) order = as_real(order, 0);
  if (bad == 4) init = as_int_matrix(init);
  if (bad == 5) { values->nrow = 0; values->ncol = 0; }
  if (setjmp(error_jmp) != 0) {
    printf("{\"registration\": \"ok\", \"error\": ");
    print_json_string(error_msg);
    printf(", \"interrupted\": %d, ", interrupted);
    print_tail();
    return 0;
  }
  SEXP out = fn(values, codes, order, init, Rf_ScalarInteger(ndim), Rf_ScalarInteger(n_iter), Rf_ScalarReal(k0),
                Rf_ScalarReal(cooling), Rf_ScalarReal(c_rep), Rf_ScalarReal(eps), Rf_ScalarInteger(window),
                Rf_ScalarInteger(freq), Rf_ScalarLogical(preserve), Rf_ScalarLogical(verbose),
                Rf_ScalarLogical(want_est));
  SEXP names = Rf_getAttrib(out, R_NamesSymbol);
  printf("{\"registration\": \"ok\", \"error\": null, \"names\": [");
  for (int i = 0; i < Rf_length(names); ++i) printf("%s\"%s\"", i ? ", " : "", CHAR(STRING_ELT(names, i)));
  printf("], \"positions\": ");
  print_reals(VECTOR_ELT(out, 0));
  printf(", \"est_distances\": ");
  print_reals(VECTOR_ELT(out, 1));
  static const char* const scalar_names[] = {"sum_abs", "count", NULL, "converged", "iterations", "final_mae", "final_k",
                                             "order_route", "numeric_max"};
  for (int q = 0; q < 9; ++q) {
    if (!scalar_names[q]) continue;
    printf(", \"%s\": ", scalar_names[q]);
    print_scalar(VECTOR_ELT(out, 2 + q));
  }
  printf(", \"order\": ");
  if (VECTOR_ELT(out, 4) == R_NilValue) printf("null");
  else print_vec(VECTOR_ELT(out, 4));
  printf(", \"interrupted\": %d, ", interrupted);
  print_tail();
  return 0;
}
