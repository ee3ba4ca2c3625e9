! The score test for binary traits through the Fortran binding: the logistic null model (mxa_assoc_logistic_null, host only) of every trait and the scan
! (mxa_assoc_score) on raw binary inputs of the working directory.  Prints checksums that do not depend on any order: the exclusive or of the 64-bit patterns
! of score, var and z, as 16 hexadecimal digits each, the sum of nobs and the sum of the Newton steps.  tests/test_fortran_assoc_score_gpu.py compares them
! with the same entries called from Python.
!
!   assoc_score_check.out <snps> <indiv> <n> <q>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding (01 = missing)
!         y.bin       indiv x n doubles, column-major: the 0 / 1 traits
!         w.bin       indiv x q doubles, column-major: the raw covariates
program assoc_score_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int) :: snps, indiv, n, q, kh, rc
 integer(c_long) :: bps, ldb, ldo
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: y(:, :), w(:, :), gam(:), res(:, :), wt(:, :), h(:, :), score(:, :), var(:, :), z(:, :)
 integer(c_int), allocatable, target :: nobs(:)
 integer(c_int), target :: iters
 type(c_ptr) :: wptr
 integer(c_int64_t) :: sum_u, sum_v, sum_z, sum_n, sum_it
 integer :: i, c, un
 character(len=64) :: arg

 if (command_argument_count() < 4) then
  print '(a)', 'usage: assoc_score_check.out <snps> <indiv> <n> <q>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) n
 call get_command_argument(4, arg); read(arg, *) q
 kh = q + 1
 bps = (int(indiv, c_long) + 3) / 4
 ldb = int(indiv, c_long) + 1
 ldo = int(snps, c_long) + 1
 allocate(plink(bps * snps), y(indiv, n), w(indiv, q), gam(kh), res(ldb, n), wt(ldb, n), h(ldb, n * kh), score(ldo, n), var(ldo, n), z(ldo, n), nobs(snps))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='y.bin', access='stream', form='unformatted', status='old', action='read'); read(un) y; close(un)
 open(newunit=un, file='w.bin', access='stream', form='unformatted', status='old', action='read'); read(un) w; close(un)
 res = -1.0_c_double
 wt = -1.0_c_double
 h = -1.0_c_double
 score = -1.0_c_double
 var = -1.0_c_double
 z = -1.0_c_double

 wptr = c_null_ptr                                  ! q = 0: no covariates, NULL (c_loc of a zero-size array is not defined)
 if (q > 0) wptr = c_loc(w)
 sum_it = 0_c_int64_t
 do c = 1, n
  rc = mxa_assoc_logistic_null(indiv, c_loc(y(1, c)), wptr, int(indiv, c_long), q, 1.0e-10_c_double, 50_c_int, c_loc(gam), c_loc(res(1, c)), c_loc(wt(1, c)), &
                               c_loc(h(1, (c - 1) * kh + 1)), ldb, c_loc(iters))
  if (rc /= 0 .or. mxa_last_error() /= 0) then
   print '(a,i0,a,i0)', 'mxa_assoc_logistic_null failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
   error stop 1
  end if
  sum_it = sum_it + iters
 end do
 rc = mxa_assoc_score(c_loc(plink), snps, indiv, c_loc(res), ldb, c_loc(wt), ldb, c_loc(h), ldb, n, kh, c_loc(score), c_loc(var), c_loc(z), ldo, c_loc(nobs))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_score failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 if (any(res(ldb, :) /= -1.0_c_double) .or. any(wt(ldb, :) /= -1.0_c_double) .or. any(h(ldb, :) /= -1.0_c_double) .or. any(score(ldo, :) /= -1.0_c_double) &
     .or. any(var(ldo, :) /= -1.0_c_double) .or. any(z(ldo, :) /= -1.0_c_double)) then
  print '(a)', 'a padding row was written'
  error stop 1
 end if
 sum_u = 0_c_int64_t
 sum_v = 0_c_int64_t
 sum_z = 0_c_int64_t
 sum_n = 0_c_int64_t
 do c = 1, n
  do i = 1, snps
   sum_u = ieor(sum_u, transfer(score(i, c), sum_u))
   sum_v = ieor(sum_v, transfer(var(i, c), sum_v))
   sum_z = ieor(sum_z, transfer(z(i, c), sum_z))
  end do
 end do
 do i = 1, snps
  sum_n = sum_n + nobs(i)
 end do
 print '(a,z16.16,a,z16.16,a,z16.16,a,i0,a,i0,a)', 'assoc_score_check: score ', sum_u, ' var ', sum_v, ' z ', sum_z, ' nobs ', sum_n, ' iters ', sum_it, ' PASS'
end program
