! The set tests through the Fortran binding: the logistic null model (mxa_assoc_logistic_null, host only) of every trait, then burden and SKAT statistics of
! SNP sets (mxa_assoc_set) and their p-values (mxa_assoc_skat_pvalue) on raw binary inputs of the working directory.  Prints checksums that do not depend on
! any order: the exclusive or of the 64-bit patterns of stat, phi, the p-values and score, as 16 hexadecimal digits each, and the sum of nobs.
! tests/test_fortran_assoc_set_gpu.py compares them with the same entries called from Python.
!
!   assoc_set_check.out <snps> <indiv> <n> <q> <nsets> <entries>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding (01 = missing)
!         y.bin       indiv x n doubles, column-major: the 0 / 1 traits
!         w.bin       indiv x q doubles, column-major: the raw covariates
!         setptr.bin  nsets + 1 64-bit integers; setidx.bin  `entries` 32-bit SNP indices, 0-based; setwt.bin  `entries` doubles
program assoc_set_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int) :: snps, indiv, n, q, kh, rc, nsets, entries
 integer(c_long) :: bps, ldb, ldo, lds, nphi, count
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: y(:, :), w(:, :), gam(:), res(:, :), wt(:, :), h(:, :), score(:, :), stat(:, :), phi(:), setwt(:), qv(:), c1(:), c2(:), &
                                        c4(:), pval(:), df(:)
 integer(c_long), allocatable, target :: setptr(:)
 integer(c_int), allocatable, target :: setidx(:), nobs(:)
 type(c_ptr) :: wptr
 integer(c_int64_t) :: sum_s, sum_f, sum_p, sum_u, sum_n
 integer :: i, c, k, un
 character(len=64) :: arg

 if (command_argument_count() < 6) then
  print '(a)', 'usage: assoc_set_check.out <snps> <indiv> <n> <q> <nsets> <entries>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) n
 call get_command_argument(4, arg); read(arg, *) q
 call get_command_argument(5, arg); read(arg, *) nsets
 call get_command_argument(6, arg); read(arg, *) entries
 kh = q + 1
 bps = (int(indiv, c_long) + 3) / 4
 ldb = int(indiv, c_long) + 1
 ldo = int(snps, c_long) + 1
 lds = int(nsets, c_long) + 1
 allocate(plink(bps * snps), y(indiv, n), w(indiv, q), gam(kh), res(ldb, n), wt(ldb, n), h(ldb, n * kh), score(ldo, n), stat(lds, 6 * n), nobs(snps), &
          setptr(nsets + 1), setidx(entries), setwt(entries))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='y.bin', access='stream', form='unformatted', status='old', action='read'); read(un) y; close(un)
 open(newunit=un, file='w.bin', access='stream', form='unformatted', status='old', action='read'); read(un) w; close(un)
 open(newunit=un, file='setptr.bin', access='stream', form='unformatted', status='old', action='read'); read(un) setptr; close(un)
 open(newunit=un, file='setidx.bin', access='stream', form='unformatted', status='old', action='read'); read(un) setidx; close(un)
 open(newunit=un, file='setwt.bin', access='stream', form='unformatted', status='old', action='read'); read(un) setwt; close(un)
 nphi = 0
 do k = 1, nsets
  nphi = nphi + int(n, c_long) * (setptr(k + 1) - setptr(k)) ** 2
 end do
 allocate(phi(nphi + 1))
 res = -1.0_c_double
 wt = -1.0_c_double
 h = -1.0_c_double
 score = -1.0_c_double
 stat = -1.0_c_double
 phi = -1.0_c_double

 wptr = c_null_ptr                                  ! q = 0: no covariates, NULL (c_loc of a zero-size array is not defined)
 if (q > 0) wptr = c_loc(w)
 do c = 1, n
  rc = mxa_assoc_logistic_null(indiv, c_loc(y(1, c)), wptr, int(indiv, c_long), q, 1.0e-10_c_double, 50_c_int, c_loc(gam), c_loc(res(1, c)), c_loc(wt(1, c)), &
                               c_loc(h(1, (c - 1) * kh + 1)), ldb, c_null_ptr)
  if (rc /= 0 .or. mxa_last_error() /= 0) then
   print '(a,i0,a,i0)', 'mxa_assoc_logistic_null failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
   error stop 1
  end if
 end do
 rc = mxa_assoc_set(c_loc(plink), snps, indiv, c_loc(res), ldb, c_loc(wt), ldb, c_loc(h), ldb, n, kh, nsets, c_loc(setptr), c_loc(setidx), c_loc(setwt), &
                    c_loc(score), c_null_ptr, c_null_ptr, ldo, c_loc(nobs), c_loc(stat), lds, c_loc(phi))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_set failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 if (any(score(ldo, :) /= -1.0_c_double) .or. any(stat(lds, :) /= -1.0_c_double) .or. phi(nphi + 1) /= -1.0_c_double) then
  print '(a)', 'a padding row was written'
  error stop 1
 end if
 count = int(nsets, c_long) * n
 allocate(qv(count), c1(count), c2(count), c4(count), pval(count), df(count))
 do c = 1, n
  do k = 1, nsets
   i = (c - 1) * nsets + k
   qv(i) = stat(k, 6 * (c - 1) + 3)
   c1(i) = stat(k, 6 * (c - 1) + 4)
   c2(i) = stat(k, 6 * (c - 1) + 5)
   c4(i) = stat(k, 6 * (c - 1) + 6)
  end do
 end do
 rc = mxa_assoc_skat_pvalue(count, c_loc(qv), c_loc(c1), c_loc(c2), c_loc(c4), c_loc(pval), c_loc(df))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_assoc_skat_pvalue failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 sum_s = 0_c_int64_t
 sum_f = 0_c_int64_t
 sum_p = 0_c_int64_t
 sum_u = 0_c_int64_t
 sum_n = 0_c_int64_t
 do c = 1, 6 * n
  do k = 1, nsets
   sum_s = ieor(sum_s, transfer(stat(k, c), sum_s))
  end do
 end do
 do i = 1, int(nphi)
  sum_f = ieor(sum_f, transfer(phi(i), sum_f))
 end do
 do i = 1, int(count)
  sum_p = ieor(sum_p, transfer(pval(i), sum_p))
 end do
 do c = 1, n
  do i = 1, snps
   sum_u = ieor(sum_u, transfer(score(i, c), sum_u))
  end do
 end do
 do i = 1, snps
  sum_n = sum_n + nobs(i)
 end do
 print '(a,z16.16,a,z16.16,a,z16.16,a,z16.16,a,i0,a)', 'assoc_set_check: stat ', sum_s, ' phi ', sum_f, ' pval ', sum_p, ' score ', sum_u, ' nobs ', sum_n, ' PASS'
end program
