! The score test with effect sizes through the Fortran binding: the logistic null model (mxa_assoc_logistic_null, host only) of every trait, the fitted
! probabilities p = y - r, and the scan with its Firth-penalised fits (mxa_assoc_score_firth) on raw binary inputs of the working directory.  Prints checksums
! that do not depend on any order: the exclusive or of the 64-bit patterns of score, z, beta, se, chisq and pval, as 16 hexadecimal digits each, the sum of the
! flags, the number of fitted items (flag 1) and the sum of nobs.  tests/test_fortran_assoc_firth_gpu.py compares them with the same entries called from Python.
!
!   assoc_firth_check.out <snps> <indiv> <n> <q> <z_cutoff> <penalty>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding (01 = missing)
!         y.bin       indiv x n doubles, column-major: the 0 / 1 traits
!         w.bin       indiv x q doubles, column-major: the raw covariates
program assoc_firth_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int) :: snps, indiv, n, q, kh, rc, penalty
 integer(c_long) :: bps, ldb, ldo
 real(c_double) :: z_cutoff
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: y(:, :), w(:, :), gam(:), res(:, :), wt(:, :), h(:, :), pfit(:, :), score(:, :), z(:, :), beta(:, :), se(:, :), &
                                        chisq(:, :), pval(:, :)
 integer(c_int), allocatable, target :: flag(:, :), nobs(:)
 type(c_ptr) :: wptr
 integer(c_int64_t) :: sum_u, sum_z, sum_b, sum_s, sum_x, sum_p, sum_f, sum_1, sum_n
 integer :: i, c, un
 character(len=64) :: arg

 if (command_argument_count() < 6) then
  print '(a)', 'usage: assoc_firth_check.out <snps> <indiv> <n> <q> <z_cutoff> <penalty>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) n
 call get_command_argument(4, arg); read(arg, *) q
 call get_command_argument(5, arg); read(arg, *) z_cutoff
 call get_command_argument(6, arg); read(arg, *) penalty
 kh = q + 1
 bps = (int(indiv, c_long) + 3) / 4
 ldb = int(indiv, c_long) + 1
 ldo = int(snps, c_long) + 1
 allocate(plink(bps * snps), y(indiv, n), w(indiv, q), gam(kh), res(ldb, n), wt(ldb, n), h(ldb, n * kh), pfit(ldb, n), score(ldo, n), z(ldo, n), beta(ldo, n), &
          se(ldo, n), chisq(ldo, n), pval(ldo, n), flag(ldo, n), nobs(snps))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='y.bin', access='stream', form='unformatted', status='old', action='read'); read(un) y; close(un)
 open(newunit=un, file='w.bin', access='stream', form='unformatted', status='old', action='read'); read(un) w; close(un)
 res = -1.0_c_double
 wt = -1.0_c_double
 h = -1.0_c_double
 pfit = -1.0_c_double
 score = -1.0_c_double
 z = -1.0_c_double
 beta = -1.0_c_double
 se = -1.0_c_double
 chisq = -1.0_c_double
 pval = -1.0_c_double
 flag = -1_c_int

 wptr = c_null_ptr                                  ! q = 0: no covariates, NULL (c_loc of a zero-size array is not defined)
 if (q > 0) wptr = c_loc(w)
 do c = 1, n
  rc = mxa_assoc_logistic_null(indiv, c_loc(y(1, c)), wptr, int(indiv, c_long), q, 1.0e-10_c_double, 50_c_int, c_loc(gam), c_loc(res(1, c)), c_loc(wt(1, c)), &
                               c_loc(h(1, (c - 1) * kh + 1)), ldb, c_null_ptr)
  if (rc /= 0 .or. mxa_last_error() /= 0) then
   print '(a,i0,a,i0)', 'mxa_assoc_logistic_null failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
   error stop 1
  end if
  pfit(1:indiv, c) = y(:, c) - res(1:indiv, c)
 end do
 rc = mxa_assoc_score_firth(c_loc(plink), snps, indiv, c_loc(pfit), ldb, c_loc(res), ldb, c_loc(wt), ldb, c_loc(h), ldb, n, kh, z_cutoff, penalty, &
                            2.0_c_double ** (-30), 50_c_int, c_loc(score), c_null_ptr, c_loc(z), c_loc(beta), c_loc(se), c_loc(chisq), c_loc(pval), ldo, &
                            c_loc(flag), c_loc(nobs))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_score_firth failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 if (any(pfit(ldb, :) /= -1.0_c_double) .or. any(score(ldo, :) /= -1.0_c_double) .or. any(z(ldo, :) /= -1.0_c_double) .or. any(beta(ldo, :) /= -1.0_c_double) &
     .or. any(se(ldo, :) /= -1.0_c_double) .or. any(chisq(ldo, :) /= -1.0_c_double) .or. any(pval(ldo, :) /= -1.0_c_double) .or. any(flag(ldo, :) /= -1_c_int)) then
  print '(a)', 'a padding row was written'
  error stop 1
 end if
 sum_u = 0_c_int64_t
 sum_z = 0_c_int64_t
 sum_b = 0_c_int64_t
 sum_s = 0_c_int64_t
 sum_x = 0_c_int64_t
 sum_p = 0_c_int64_t
 sum_f = 0_c_int64_t
 sum_1 = 0_c_int64_t
 sum_n = 0_c_int64_t
 do c = 1, n
  do i = 1, snps
   sum_u = ieor(sum_u, transfer(score(i, c), sum_u))
   sum_z = ieor(sum_z, transfer(z(i, c), sum_z))
   sum_b = ieor(sum_b, transfer(beta(i, c), sum_b))
   sum_s = ieor(sum_s, transfer(se(i, c), sum_s))
   sum_x = ieor(sum_x, transfer(chisq(i, c), sum_x))
   sum_p = ieor(sum_p, transfer(pval(i, c), sum_p))
   sum_f = sum_f + flag(i, c)
   if (flag(i, c) == 1) sum_1 = sum_1 + 1
  end do
 end do
 do i = 1, snps
  sum_n = sum_n + nobs(i)
 end do
 print '(a,z16.16,a,z16.16,a,z16.16,a,z16.16,a,z16.16,a,z16.16,a,i0,a,i0,a,i0,a)', 'assoc_firth_check: score ', sum_u, ' z ', sum_z, ' beta ', sum_b, ' se ', sum_s, &
       ' chisq ', sum_x, ' pval ', sum_p, ' flags ', sum_f, ' fitted ', sum_1, ' nobs ', sum_n, ' PASS'
end program
