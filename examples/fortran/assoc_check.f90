! The association scan through the Fortran binding: the covariate basis (mxa_assoc_basis, host only) and the scan (mxa_assoc_linear) on raw binary inputs of the
! working directory.  Prints checksums that do not depend on any order: the exclusive or of the 64-bit patterns of beta, se and t, as 16 hexadecimal digits
! each, the sum of nobs and dof.  tests/test_fortran_assoc_gpu.py compares them with the same entries called from Python.
!
!   assoc_check.out <snps> <indiv> <n> <k>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding (01 = missing)
!         y.bin       ldy x n doubles, column-major, ldy = indiv + 2 (the two rows behind a column are not read)
!         w.bin       indiv x k doubles, column-major: the raw covariates
program assoc_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int) :: snps, indiv, n, k, rc
 integer(c_long) :: bps, ldy, ldq, ldo
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: y(:, :), w(:, :), q(:, :), beta(:, :), se(:, :), t(:, :)
 integer(c_int), allocatable, target :: nobs(:)
 integer(c_int), target :: dof
 integer(c_int64_t) :: sum_b, sum_s, sum_t, sum_n
 integer :: i, c, un
 character(len=64) :: arg

 if (command_argument_count() < 4) then
  print '(a)', 'usage: assoc_check.out <snps> <indiv> <n> <k>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) n
 call get_command_argument(4, arg); read(arg, *) k
 bps = (int(indiv, c_long) + 3) / 4
 ldy = int(indiv, c_long) + 2
 ldq = int(indiv, c_long) + 1
 ldo = int(snps, c_long) + 1
 allocate(plink(bps * snps), y(ldy, n), w(indiv, k), q(ldq, k), beta(ldo, n), se(ldo, n), t(ldo, n), nobs(snps))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='y.bin', access='stream', form='unformatted', status='old', action='read'); read(un) y; close(un)
 open(newunit=un, file='w.bin', access='stream', form='unformatted', status='old', action='read'); read(un) w; close(un)
 q = -1.0_c_double
 beta = -1.0_c_double
 se = -1.0_c_double
 t = -1.0_c_double

 rc = mxa_assoc_basis(indiv, c_loc(w), int(indiv, c_long), k, c_loc(q), ldq)
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_basis failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 rc = mxa_assoc_linear(c_loc(plink), snps, indiv, c_loc(y), ldy, n, c_loc(q), ldq, k, c_loc(beta), c_loc(se), c_loc(t), ldo, c_loc(nobs), c_loc(dof))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_linear failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 if (any(q(ldq, :) /= -1.0_c_double) .or. any(beta(ldo, :) /= -1.0_c_double) .or. any(se(ldo, :) /= -1.0_c_double) .or. any(t(ldo, :) /= -1.0_c_double)) then
  print '(a)', 'a padding row was written'
  error stop 1
 end if
 sum_b = 0_c_int64_t
 sum_s = 0_c_int64_t
 sum_t = 0_c_int64_t
 sum_n = 0_c_int64_t
 do c = 1, n
  do i = 1, snps
   sum_b = ieor(sum_b, transfer(beta(i, c), sum_b))
   sum_s = ieor(sum_s, transfer(se(i, c), sum_s))
   sum_t = ieor(sum_t, transfer(t(i, c), sum_t))
  end do
 end do
 do i = 1, snps
  sum_n = sum_n + nobs(i)
 end do
 print '(a,z16.16,a,z16.16,a,z16.16,a,i0,a,i0,a)', 'assoc_check: beta ', sum_b, ' se ', sum_s, ' t ', sum_t, ' nobs ', sum_n, ' dof ', dof, ' PASS'
end program
