! The window applied to a matrix through the Fortran binding: mxa_ld_window_apply called once through modmiraculix_amd with n = 2 columns, on raw binary inputs
! of the working directory.  Prints a checksum of Y that does not depend on any order: the exclusive or of the 64-bit patterns of its snps x 2 values, as 16
! hexadecimal digits.  tests/test_fortran_ld_apply_gpu.py compares it with the same entry called from Python.
!
!   ld_apply_check.out <snps> <indiv> <term>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding, no missing code
!         f.bin       snps doubles: allele frequencies
!         last.bin    snps 32-bit integers: the window ends (0-based)
!         x.bin       ldx x 2 doubles, column-major, ldx = snps + 2 (the two rows behind a column are not read)
program ld_apply_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int), parameter :: n = 2
 integer(c_int) :: snps, indiv, term, rc
 integer(c_long) :: bps, ldx, ldy
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: f(:), x(:, :), y(:, :)
 integer(c_int), allocatable, target :: last(:)
 integer(c_int64_t) :: sum_bits
 integer :: i, c, un
 character(len=64) :: arg

 if (command_argument_count() < 3) then
  print '(a)', 'usage: ld_apply_check.out <snps> <indiv> <term>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) term
 bps = (int(indiv, c_long) + 3) / 4
 ldx = int(snps, c_long) + 2
 ldy = int(snps, c_long) + 1
 allocate(plink(bps * snps), f(snps), last(snps), x(ldx, n), y(ldy, n))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='f.bin', access='stream', form='unformatted', status='old', action='read'); read(un) f; close(un)
 open(newunit=un, file='last.bin', access='stream', form='unformatted', status='old', action='read'); read(un) last; close(un)
 open(newunit=un, file='x.bin', access='stream', form='unformatted', status='old', action='read'); read(un) x; close(un)
 y = -1.0_c_double

 rc = mxa_ld_window_apply(c_loc(plink), snps, indiv, c_loc(last), term, c_loc(x), ldx, n, c_loc(y), ldy, 1_c_int, c_loc(f))
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_ld_window_apply failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 if (y(ldy, 1) /= -1.0_c_double .or. y(ldy, 2) /= -1.0_c_double) then
  print '(a)', 'the padding row of y was written'
  error stop 1
 end if
 sum_bits = 0_c_int64_t
 do c = 1, n
  do i = 1, snps
   sum_bits = ieor(sum_bits, transfer(y(i, c), sum_bits))
  end do
 end do
 print '(a,z16.16,a)', 'ld_apply_check: checksum ', sum_bits, ' PASS'
end program
