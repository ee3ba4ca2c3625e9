! Fortran binding of libmiraculix_amd.so: what a maintainer of the reference would put beside src/bindings/Fortran/mod5codesapi.f90 to reach the ADDITIVE
! entry points of include/miraculix_amd.h (part 2) from Fortran.  The five reference entries keep the interfaces of mod5codesapi.f90:22-82 (same C
! symbols, same argument kinds) and are repeated here under the same names so that a program needs this one module only.
! Conventions: `compressed` is the opaque object (type(c_ptr)); leading dimensions of the mxa_* entries are C long (integer(c_long)); file names are
! NUL-terminated character arrays (trim(name)//c_null_char); optional C pointers are passed as type(c_ptr) by value (c_loc(x) or c_null_ptr).
! Built and run by tests/test_fortran_binding_gpu.py through examples/fortran/gblup_cg.f90.
module modmiraculix_amd
 use, intrinsic :: iso_c_binding, only: c_int, c_long, c_double, c_char, c_ptr
 implicit none
 private
 ! reference entries (5codesAPI.c:37-161)
 public :: c_setOptions_compressed, c_plink2compressed, c_dgemm_compressed, c_get_compressed_freq, c_free_compressed
 ! additive entries
 public :: mxa_last_error, mxa_device_count, mxa_bed2compressed, mxa_gram_matvec, mxa_set_engine, mxa_get_engine, mxa_last_path
 public :: mxa_single_orientation, mxa_num_shards, mxa_allele_freq, mxa_transpose_2bit
 public :: mxa_plink2compressed_begin, mxa_plink2compressed_rows, mxa_plink2compressed_end
 public :: mxa_ld_band, mxa_ld_scores
 public :: mxa_ld_band_pairwise, mxa_ld_scores_pairwise
 public :: mxa_ld_window_bounds, mxa_ld_window_rows, mxa_ld_window_scores, mxa_ld_window_rows_pairwise, mxa_ld_window_scores_pairwise
 public :: mxa_ld_window_pairs, mxa_ld_window_pairs_pairwise
 public :: mxa_ld_prune_csr, mxa_ld_window_prune, mxa_ld_window_prune_pairwise
 public :: mxa_ld_window_apply, mxa_ld_window_apply_pairwise
 public :: mxa_ld_op_bytes, mxa_ld_op_create, mxa_ld_op_create_pairwise, mxa_ld_op_from_rows, mxa_ld_op_rows, mxa_ld_op_apply, mxa_ld_op_solve, mxa_ld_op_free
 public :: mxa_assoc_basis, mxa_assoc_linear
 public :: mxa_assoc_score, mxa_assoc_logistic_null
 public :: mxa_assoc_score_spa
 public :: mxa_assoc_score_firth
 public :: mxa_assoc_set, mxa_assoc_skat_pvalue

 interface
  subroutine c_setOptions_compressed(use_gpu, cores, floatLoop, meanSubstract, ignore_missings, do_not_center, do_normalize, use_miraculix_freq, variant, print_details) &
             bind(C, name='setOptions_compressed')
   import c_int
   integer(c_int), value, intent(in) :: use_gpu, cores, floatLoop, meanSubstract, ignore_missings, do_not_center, do_normalize, use_miraculix_freq, variant, print_details
  end subroutine

  subroutine c_plink2compressed(plink, plink_transposed, snps, indiv, f, n, compressed) bind(C, name='plink2compressed')
   import c_int, c_ptr, c_double
   type(c_ptr), value, intent(in) :: plink, plink_transposed      ! plink_transposed may be c_null_ptr: one packed copy is kept anyway
   integer(c_int), value, intent(in) :: snps, indiv, n
   real(c_double), intent(in) :: f(*)
   type(c_ptr), intent(out) :: compressed
  end subroutine

  subroutine c_dgemm_compressed(trans, compressed, n, B, ldb, C, ldc) bind(C, name='dgemm_compressed')
   import c_char, c_int, c_double, c_ptr
   character(c_char), intent(in) :: trans(*)
   type(c_ptr), value, intent(in) :: compressed
   integer(c_int), value, intent(in) :: n, ldb, ldc
   real(c_double), intent(in) :: B(ldb, *)
   real(c_double), intent(inout) :: C(ldc, *)
  end subroutine

  subroutine c_get_compressed_freq(compressed, freq) bind(C, name='get_compressed_freq')
   import c_double, c_ptr
   type(c_ptr), value, intent(in) :: compressed
   real(c_double), intent(out) :: freq(*)
  end subroutine

  subroutine c_free_compressed(compressed) bind(C, name='free_compressed')
   import c_ptr
   type(c_ptr), intent(inout) :: compressed                          ! c_null_ptr afterwards
  end subroutine

  ! ---- additive (include/miraculix_amd.h part 2)
  function mxa_last_error() bind(C, name='mxa_last_error') result(code)   ! 0 = the most recent fallible call succeeded
   import c_int
   integer(c_int) :: code
  end function

  function mxa_device_count() bind(C, name='mxa_device_count') result(n)
   import c_int
   integer(c_int) :: n
  end function

  ! .bed staging owned by the library; snps / indiv <= 0: from the line counts of the .bim / .fam next to the file.  f_out: c_loc of snps doubles, or c_null_ptr
  function mxa_bed2compressed(bed_path, snps, indiv, max_n, compressed, f_out, snps_out, indiv_out) bind(C, name='mxa_bed2compressed') result(rc)
   import c_char, c_int, c_ptr
   character(c_char), intent(in) :: bed_path(*)
   integer(c_int), value, intent(in) :: snps, indiv, max_n
   type(c_ptr), intent(out) :: compressed
   type(c_ptr), value, intent(in) :: f_out
   integer(c_int), intent(out) :: snps_out, indiv_out
   integer(c_int) :: rc
  end function

  ! out (indiv x n) = Zc (Zc^T V): one step of the GRM solvers, the snps x n intermediate stays on the device
  function mxa_gram_matvec(compressed, n, V, ldv, out, ldo) bind(C, name='mxa_gram_matvec') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: compressed
   integer(c_int), value, intent(in) :: n
   integer(c_long), value, intent(in) :: ldv, ldo
   real(c_double), intent(in) :: V(ldv, *)
   real(c_double), intent(inout) :: out(ldo, *)
   integer(c_int) :: rc
  end function

  function mxa_set_engine(engine) bind(C, name='mxa_set_engine') result(previous)   ! 0 default, 1 i8, 3 f64-strict, 4 i8-exact
   import c_int
   integer(c_int), value, intent(in) :: engine
   integer(c_int) :: previous
  end function

  function mxa_get_engine() bind(C, name='mxa_get_engine') result(engine)
   import c_int
   integer(c_int) :: engine
  end function

  function mxa_last_path() bind(C, name='mxa_last_path') result(path)               ! 0 k_gemm, 1 k_lut, 2 k_gemm_i8, 3 fp64 chains behind the int8 route
   import c_int
   integer(c_int) :: path
  end function

  function mxa_single_orientation(compressed) bind(C, name='mxa_single_orientation') result(single)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: compressed
   integer(c_int) :: single
  end function

  function mxa_num_shards(compressed) bind(C, name='mxa_num_shards') result(shards)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: compressed
   integer(c_int) :: shards
  end function

  function mxa_allele_freq(plink, snps, indiv, f) bind(C, name='mxa_allele_freq') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink
   integer(c_long), value, intent(in) :: snps, indiv
   real(c_double), intent(out) :: f(*)
   integer(c_int) :: rc
  end function

  function mxa_transpose_2bit(in, rows, cols, out) bind(C, name='mxa_transpose_2bit') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: in, out
   integer(c_long), value, intent(in) :: rows, cols
   integer(c_int) :: rc
  end function

  ! windowed LD (plink = snps rows of ceil(indiv/4) bytes, host or device like every pointer here; window = neighbours on each side, 0 <= window < snps):
  ! band(d + 1, i + 1) = R(i, i + d), 0 <= d <= window -- a (ldb, snps) array in LAPACK's lower symmetric band storage (dsbmv / dpbtrf 'L'); kind 0: r, 1: r^2
  function mxa_ld_band(plink, snps, indiv, window, band, ldb, kind, is_plink_format, allele_freq) bind(C, name='mxa_ld_band') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, band, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, window, kind, is_plink_format
   integer(c_long), value, intent(in) :: ldb
   integer(c_int) :: rc
  end function
  ! scores(i + 1) = sum over |i - j| <= window of r_ij^2 (adjust = 1: of r^2 - (1 - r^2) / (indiv - 2)); the band is never written
  function mxa_ld_scores(plink, snps, indiv, window, scores, adjust, is_plink_format, allele_freq) bind(C, name='mxa_ld_scores') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, scores, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, window, adjust, is_plink_format
   integer(c_int) :: rc
  end function

  ! the same two on data with missing genotypes (PLINK code 01): the pairwise-complete r, Pearson's r over the individuals genotyped at both SNPs.
  ! PLINK coding only, no allele frequencies; band / scores laid out as above; adjust = 1 uses the pair's own count N_ij in r^2 - (1 - r^2) / (N_ij - 2)
  function mxa_ld_band_pairwise(plink, snps, indiv, window, band, ldb, kind) bind(C, name='mxa_ld_band_pairwise') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, band
   integer(c_int), value, intent(in) :: snps, indiv, window, kind
   integer(c_long), value, intent(in) :: ldb
   integer(c_int) :: rc
  end function
  function mxa_ld_scores_pairwise(plink, snps, indiv, window, scores, adjust) bind(C, name='mxa_ld_scores_pairwise') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, scores
   integer(c_int), value, intent(in) :: snps, indiv, window, adjust
   integer(c_int) :: rc
  end function

  ! windows by distance: the window of SNP i (0-based) ends at last(i + 1), i <= last <= snps - 1, non-decreasing.  mxa_ld_window_bounds (host only) makes
  ! last -- and rowptr, snps + 1 C longs, the exclusive prefix sum of last(i + 1) - i + 1 -- from positions (base pairs or centimorgans; c_null_ptr: none),
  ! chromosome codes (c_null_ptr: one chromosome), max_dist and max_snps (< 0: none).  rows(rowptr(i + 1) + d + 1) = R(i, i + d), 0 <= d <= last(i + 1) - i;
  ! scores as mxa_ld_scores over the window; the _pairwise pair on data with missing genotypes.  last: host or device, c_loc of integer(c_int).
  function mxa_ld_window_bounds(snps, pos, chrom, max_dist, max_snps, last, rowptr) bind(C, name='mxa_ld_window_bounds') result(rc)
   import c_int, c_double, c_ptr
   integer(c_int), value, intent(in) :: snps, max_snps
   type(c_ptr), value, intent(in) :: pos, chrom, last, rowptr
   real(c_double), value, intent(in) :: max_dist
   integer(c_int) :: rc
  end function
  function mxa_ld_window_rows(plink, snps, indiv, last, rows, kind, is_plink_format, allele_freq) bind(C, name='mxa_ld_window_rows') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, rows, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, kind, is_plink_format
   integer(c_int) :: rc
  end function
  function mxa_ld_window_scores(plink, snps, indiv, last, scores, adjust, is_plink_format, allele_freq) bind(C, name='mxa_ld_window_scores') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, scores, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, adjust, is_plink_format
   integer(c_int) :: rc
  end function
  function mxa_ld_window_rows_pairwise(plink, snps, indiv, last, rows, kind) bind(C, name='mxa_ld_window_rows_pairwise') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, rows
   integer(c_int), value, intent(in) :: snps, indiv, kind
   integer(c_int) :: rc
  end function
  function mxa_ld_window_scores_pairwise(plink, snps, indiv, last, scores, adjust) bind(C, name='mxa_ld_window_scores_pairwise') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, scores
   integer(c_int), value, intent(in) :: snps, indiv, adjust
   integer(c_int) :: rc
  end function

  ! the pairs i < j <= last(i + 1) of a window with r * r >= min_r2 as CSR, 0-based as in C: rowptr (snps + 1 C longs), col (C ints, ascending in a row), val
  ! (kind 0: r, 1: r * r), `capacity` entries each; total: c_loc of an integer(c_long) on the host.  col = val = c_null_ptr: the count-only call (rowptr and
  ! total).  rc = 1 with mxa_last_error() = 25: total > capacity (rowptr and total are valid).  rowptr, col, val: all host or all device.
  function mxa_ld_window_pairs(plink, snps, indiv, last, min_r2, kind, rowptr, col, val, capacity, total, is_plink_format, allele_freq) &
      bind(C, name='mxa_ld_window_pairs') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, rowptr, col, val, total, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, kind, is_plink_format
   real(c_double), value, intent(in) :: min_r2
   integer(c_long), value, intent(in) :: capacity
   integer(c_int) :: rc
  end function
  function mxa_ld_window_pairs_pairwise(plink, snps, indiv, last, min_r2, kind, rowptr, col, val, capacity, total) &
      bind(C, name='mxa_ld_window_pairs_pairwise') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, rowptr, col, val, total
   integer(c_int), value, intent(in) :: snps, indiv, kind
   real(c_double), value, intent(in) :: min_r2
   integer(c_long), value, intent(in) :: capacity
   integer(c_int) :: rc
  end function

  ! LD pruning / clumping: the greedy selection on the pairs graph (edges: the pairs above; order: smaller priority first, ties by index; priority =
  ! c_null_ptr: index order).  keep: snps bytes of 0 / 1; owner (c_null_ptr skips it): snps C ints, 0-based, the index SNP of a dropped SNP's clump; keep
  ! and owner both host or both device.  n_kept: c_loc of an integer(c_long), rounds (or c_null_ptr): c_loc of an integer(c_int), both on the host.
  function mxa_ld_prune_csr(snps, rowptr, col, priority, keep, owner, n_kept, rounds) bind(C, name='mxa_ld_prune_csr') result(rc)
   import c_int, c_ptr
   integer(c_int), value, intent(in) :: snps
   type(c_ptr), value, intent(in) :: rowptr, col, priority, keep, owner, n_kept, rounds
   integer(c_int) :: rc
  end function
  function mxa_ld_window_prune(plink, snps, indiv, last, min_r2, priority, keep, owner, n_kept, rounds, is_plink_format, allele_freq) &
      bind(C, name='mxa_ld_window_prune') result(rc)
   import c_int, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, priority, keep, owner, n_kept, rounds, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, is_plink_format
   real(c_double), value, intent(in) :: min_r2
   integer(c_int) :: rc
  end function
  function mxa_ld_window_prune_pairwise(plink, snps, indiv, last, min_r2, priority, keep, owner, n_kept, rounds) &
      bind(C, name='mxa_ld_window_prune_pairwise') result(rc)
   import c_int, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, priority, keep, owner, n_kept, rounds
   integer(c_int), value, intent(in) :: snps, indiv
   real(c_double), value, intent(in) :: min_r2
   integer(c_int) :: rc
  end function

  ! the window applied to a matrix: Y = T_w(R) X, X and Y snps x n column-major (Fortran arrays x(ldx, n), y(ldy, n)), host or device each; term 0: r,
  ! 1: r * r, 2: the adjusted term of the scores.  Rows beyond snps of y are not written.  Every sum runs in a fixed order (the same bits for every n).
  function mxa_ld_window_apply(plink, snps, indiv, last, term, X, ldx, n, Y, ldy, is_plink_format, allele_freq) bind(C, name='mxa_ld_window_apply') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, X, Y, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, term, n, is_plink_format
   integer(c_long), value, intent(in) :: ldx, ldy
   integer(c_int) :: rc
  end function
  function mxa_ld_window_apply_pairwise(plink, snps, indiv, last, term, X, ldx, n, Y, ldy) bind(C, name='mxa_ld_window_apply_pairwise') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, X, Y
   integer(c_int), value, intent(in) :: snps, indiv, term, n
   integer(c_long), value, intent(in) :: ldx, ldy
   integer(c_int) :: rc
  end function

  ! the LD operator object: the window's values staged once on the device (op: a handle, type(c_ptr)), then Y = shift X + T X and the conjugate-gradient solve
  ! of (T + shift I) X = B there; iters, relres, status of the solve: host arrays of n, or c_null_ptr
  function mxa_ld_op_bytes(snps, last, entries, bytes) bind(C, name='mxa_ld_op_bytes') result(rc)
   import c_int, c_long, c_ptr
   integer(c_int), value, intent(in) :: snps
   type(c_ptr), value, intent(in) :: last
   integer(c_long), intent(out) :: entries, bytes
   integer(c_int) :: rc
  end function
  function mxa_ld_op_create(plink, snps, indiv, last, kind, is_plink_format, allele_freq, op) bind(C, name='mxa_ld_op_create') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last, allele_freq
   integer(c_int), value, intent(in) :: snps, indiv, kind, is_plink_format
   type(c_ptr), intent(out) :: op
   integer(c_int) :: rc
  end function
  function mxa_ld_op_create_pairwise(plink, snps, indiv, last, kind, op) bind(C, name='mxa_ld_op_create_pairwise') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: plink, last
   integer(c_int), value, intent(in) :: snps, indiv, kind
   type(c_ptr), intent(out) :: op
   integer(c_int) :: rc
  end function
  function mxa_ld_op_from_rows(snps, last, rows, op) bind(C, name='mxa_ld_op_from_rows') result(rc)
   import c_int, c_ptr
   integer(c_int), value, intent(in) :: snps
   type(c_ptr), value, intent(in) :: last, rows
   type(c_ptr), intent(out) :: op
   integer(c_int) :: rc
  end function
  function mxa_ld_op_rows(op, rows) bind(C, name='mxa_ld_op_rows') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: op, rows
   integer(c_int) :: rc
  end function
  function mxa_ld_op_apply(op, shift, X, ldx, n, Y, ldy) bind(C, name='mxa_ld_op_apply') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: op, X, Y
   real(c_double), value, intent(in) :: shift
   integer(c_long), value, intent(in) :: ldx, ldy
   integer(c_int), value, intent(in) :: n
   integer(c_int) :: rc
  end function
  function mxa_ld_op_solve(op, shift, B, ldb, n, X, ldx, tol, max_iter, iters, relres, status) bind(C, name='mxa_ld_op_solve') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: op, B, X, iters, relres, status
   real(c_double), value, intent(in) :: shift, tol
   integer(c_long), value, intent(in) :: ldb, ldx
   integer(c_int), value, intent(in) :: n, max_iter
   integer(c_int) :: rc
  end function
  subroutine mxa_ld_op_free(op) bind(C, name='mxa_ld_op_free')
   import c_ptr
   type(c_ptr), intent(inout) :: op
  end subroutine

  ! association scan: beta, se, t of y_c ~ 1 + Q + x_s for every SNP s (missing calls imputed by the SNP's mean); Q from mxa_assoc_basis (host only), or
  ! c_null_ptr with k = 0; beta, se, tstat: snps x n, ld ldo, each c_loc or c_null_ptr (one at least); nobs: snps ints or c_null_ptr; dof: c_loc of one int or c_null_ptr
  function mxa_assoc_basis(indiv, W, ldw, ncov, Q, ldq) bind(C, name='mxa_assoc_basis') result(rc)   ! ncov: the header's q (Fortran does not tell q from Q)
   import c_int, c_long, c_ptr
   integer(c_int), value, intent(in) :: indiv, ncov
   type(c_ptr), value, intent(in) :: W, Q
   integer(c_long), value, intent(in) :: ldw, ldq
   integer(c_int) :: rc
  end function
  function mxa_assoc_linear(plink, snps, indiv, Y, ldy, n, Q, ldq, k, beta, se, tstat, ldo, nobs, dof) bind(C, name='mxa_assoc_linear') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, Y, Q, beta, se, tstat, nobs, dof
   integer(c_int), value, intent(in) :: snps, indiv, n, k
   integer(c_long), value, intent(in) :: ldy, ldq, ldo
   integer(c_int) :: rc
  end function
  ! score test for binary traits: score, var, zstat (snps x n, ld ldo, each c_loc or c_null_ptr, one at least) from the null residuals R, the working weights
  ! Wt (indiv x n each) and the projection columns H (indiv x n kh; c_null_ptr with kh = 0); nobs: snps ints or c_null_ptr
  function mxa_assoc_score(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, score, var, zstat, ldo, nobs) bind(C, name='mxa_assoc_score') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, R, Wt, H, score, var, zstat, nobs
   integer(c_int), value, intent(in) :: snps, indiv, n, kh
   integer(c_long), value, intent(in) :: ldr, ldw, ldh, ldo
   integer(c_int) :: rc
  end function
  ! the logistic null model (host only): gamma (ncov + 1), resid = y - p, wt = p (1 - p), Hmat (indiv x (ncov + 1), ld ldh) for mxa_assoc_score with kh = ncov + 1;
  ! Wcov: indiv x ncov raw covariates or c_null_ptr with ncov = 0; iters: c_loc of one int or c_null_ptr.  (ncov, Wcov, resid, wt, Hmat: the header's q, W, r, w, H)
  function mxa_assoc_logistic_null(indiv, y, Wcov, ldw, ncov, tol, max_iter, gamma, resid, wt, Hmat, ldh, iters) bind(C, name='mxa_assoc_logistic_null') result(rc)
   import c_int, c_long, c_double, c_ptr
   integer(c_int), value, intent(in) :: indiv, ncov, max_iter
   type(c_ptr), value, intent(in) :: y, Wcov, gamma, resid, wt, Hmat, iters
   integer(c_long), value, intent(in) :: ldw, ldh
   real(c_double), value, intent(in) :: tol
   integer(c_int) :: rc
  end function

  ! the score test with saddlepoint p-values: Pfit = the null's fitted probabilities (indiv x n, ld ldp); pval (required) and flag (c_loc of snps x n ints or
  ! c_null_ptr) have the leading dimension ldo of score, var and zstat
  function mxa_assoc_score_spa(plink, snps, indiv, Pfit, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, tol, max_iter, score, var, zstat, pval, ldo, flag, nobs) &
           bind(C, name='mxa_assoc_score_spa') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, Pfit, R, Wt, H, score, var, zstat, pval, flag, nobs
   integer(c_int), value, intent(in) :: snps, indiv, n, kh, max_iter
   integer(c_long), value, intent(in) :: ldp, ldr, ldw, ldh, ldo
   real(c_double), value, intent(in) :: z_cutoff, tol
   integer(c_int) :: rc
  end function

  ! the score test with effect sizes: beta (required), se, chisq, pval (c_loc or c_null_ptr each) and flag (c_loc of snps x n ints or c_null_ptr) have the
  ! leading dimension ldo of score, var and zstat; penalty 0: maximum likelihood, 1: Firth's penalty
  function mxa_assoc_score_firth(plink, snps, indiv, Pfit, ldp, R, ldr, Wt, ldw, H, ldh, n, kh, z_cutoff, penalty, tol, max_iter, score, var, zstat, beta, se, &
           chisq, pval, ldo, flag, nobs) bind(C, name='mxa_assoc_score_firth') result(rc)
   import c_int, c_long, c_double, c_ptr
   type(c_ptr), value, intent(in) :: plink, Pfit, R, Wt, H, score, var, zstat, beta, se, chisq, pval, flag, nobs
   integer(c_int), value, intent(in) :: snps, indiv, n, kh, penalty, max_iter
   integer(c_long), value, intent(in) :: ldp, ldr, ldw, ldh, ldo
   real(c_double), value, intent(in) :: z_cutoff, tol
   integer(c_int) :: rc
  end function

  ! set-based association (burden and SKAT): set_ptr (c_loc of nsets + 1 c_long), set_idx (c_loc of c_int, 0-based SNP indices) and set_wt (c_loc of doubles or
  ! c_null_ptr) are a CSR list on the host; score, var, zstat and nobs are c_loc or c_null_ptr each; stat (required): nsets x 6 n doubles, ld lds; phi: c_loc
  ! of n sum m_k^2 doubles or c_null_ptr
  function mxa_assoc_set(plink, snps, indiv, R, ldr, Wt, ldw, H, ldh, n, kh, nsets, set_ptr, set_idx, set_wt, score, var, zstat, ldo, nobs, stat, lds, phi) &
           bind(C, name='mxa_assoc_set') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: plink, R, Wt, H, set_ptr, set_idx, set_wt, score, var, zstat, nobs, stat, phi
   integer(c_int), value, intent(in) :: snps, indiv, n, kh, nsets
   integer(c_long), value, intent(in) :: ldr, ldw, ldh, ldo, lds
   integer(c_int) :: rc
  end function

  ! the SKAT p-values of count items from (Q, c1, c2, c4), on the host; df: c_loc of count doubles or c_null_ptr
  function mxa_assoc_skat_pvalue(count, Q, c1, c2, c4, pval, df) bind(C, name='mxa_assoc_skat_pvalue') result(rc)
   import c_int, c_long, c_ptr
   integer(c_long), value, intent(in) :: count
   type(c_ptr), value, intent(in) :: Q, c1, c2, c4, pval, df
   integer(c_int) :: rc
  end function

  ! incremental staging: the object is filled by blocks of SNP rows (objects larger than any buffer the caller could hold)
  function mxa_plink2compressed_begin(snps, indiv, max_n, compressed) bind(C, name='mxa_plink2compressed_begin') result(rc)
   import c_int, c_long, c_ptr
   integer(c_long), value, intent(in) :: snps, indiv
   integer(c_int), value, intent(in) :: max_n
   type(c_ptr), intent(out) :: compressed
   integer(c_int) :: rc
  end function

  function mxa_plink2compressed_rows(compressed, plink_rows, snp_begin, nrows, f_rows) bind(C, name='mxa_plink2compressed_rows') result(rc)
   import c_int, c_long, c_ptr
   type(c_ptr), value, intent(in) :: compressed, plink_rows, f_rows   ! f_rows: c_loc of nrows doubles, or c_null_ptr (counted on the device)
   integer(c_long), value, intent(in) :: snp_begin, nrows              ! zero-based first row
   integer(c_int) :: rc
  end function

  function mxa_plink2compressed_end(compressed) bind(C, name='mxa_plink2compressed_end') result(rc)
   import c_int, c_ptr
   type(c_ptr), value, intent(in) :: compressed
   integer(c_int) :: rc
  end function
 end interface
end module modmiraculix_amd
