! The LD operator object through the Fortran binding: created once from raw binary inputs of the working directory, applied with n = 2 columns and a shift,
! then ridge-solved on the same two columns.  Prints two checksums that do not depend on any order: the exclusive or of the 64-bit patterns of Y and of the
! solution X, as 16 hexadecimal digits each, and the iteration counts.  tests/test_fortran_ld_op_gpu.py compares them with the same entries called from Python.
!
!   ld_op_check.out <snps> <indiv> <kind>
! reads   plink.bin   snps rows of ceil(indiv / 4) bytes, PLINK coding, no missing code
!         f.bin       snps doubles: allele frequencies
!         last.bin    snps 32-bit integers: the window ends (0-based)
!         x.bin       ldx x 2 doubles, column-major, ldx = snps + 2 (the two rows behind a column are not read)
program ld_op_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int), parameter :: n = 2
 real(c_double), parameter :: shift_apply = 0.25_c_double, shift_solve = 2.0_c_double, tol = 1.0e-10_c_double
 integer(c_int) :: snps, indiv, kind, rc
 integer(c_long) :: bps, ldx, ldy, entries, nbytes
 integer(c_int8_t), allocatable, target :: plink(:)
 real(c_double), allocatable, target :: f(:), x(:, :), y(:, :), sol(:, :)
 real(c_double), target :: relres(n)
 integer(c_int), allocatable, target :: last(:)
 integer(c_int), target :: iters(n), status(n)
 type(c_ptr) :: op
 integer(c_int64_t) :: sum_y, sum_x
 integer :: i, c, un
 character(len=64) :: arg

 if (command_argument_count() < 3) then
  print '(a)', 'usage: ld_op_check.out <snps> <indiv> <kind>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) kind
 bps = (int(indiv, c_long) + 3) / 4
 ldx = int(snps, c_long) + 2
 ldy = int(snps, c_long) + 1
 allocate(plink(bps * snps), f(snps), last(snps), x(ldx, n), y(ldy, n), sol(ldy, n))
 open(newunit=un, file='plink.bin', access='stream', form='unformatted', status='old', action='read'); read(un) plink; close(un)
 open(newunit=un, file='f.bin', access='stream', form='unformatted', status='old', action='read'); read(un) f; close(un)
 open(newunit=un, file='last.bin', access='stream', form='unformatted', status='old', action='read'); read(un) last; close(un)
 open(newunit=un, file='x.bin', access='stream', form='unformatted', status='old', action='read'); read(un) x; close(un)
 y = -1.0_c_double
 sol = -1.0_c_double

 rc = mxa_ld_op_bytes(snps, c_loc(last), entries, nbytes)
 if (rc /= 0 .or. nbytes < 8 * (2 * entries - snps)) then
  print '(a,i0)', 'mxa_ld_op_bytes failed: rc ', rc
  error stop 1
 end if
 op = c_null_ptr
 rc = mxa_ld_op_create(c_loc(plink), snps, indiv, c_loc(last), kind, 1_c_int, c_loc(f), op)
 if (rc /= 0 .or. .not. c_associated(op)) then
  print '(a,i0,a,i0)', 'mxa_ld_op_create failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 rc = mxa_ld_op_apply(op, shift_apply, c_loc(x), ldx, n, c_loc(y), ldy)
 if (rc /= 0 .or. mxa_last_error() /= 0) then
  print '(a,i0,a,i0)', 'mxa_ld_op_apply failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
  error stop 1
 end if
 rc = mxa_ld_op_solve(op, shift_solve, c_loc(x), ldx, n, c_loc(sol), ldy, tol, 1000_c_int, c_loc(iters), c_loc(relres), c_loc(status))
 if (rc /= 0 .or. mxa_last_error() /= 0 .or. any(status /= 0) .or. any(relres > tol)) then
  print '(a,i0,a,i0,a,2i2)', 'mxa_ld_op_solve failed: rc ', rc, ', mxa_last_error ', mxa_last_error(), ', status ', status
  error stop 1
 end if
 call mxa_ld_op_free(op)
 if (c_associated(op)) then
  print '(a)', 'mxa_ld_op_free left the handle set'
  error stop 1
 end if
 if (y(ldy, 1) /= -1.0_c_double .or. y(ldy, 2) /= -1.0_c_double .or. sol(ldy, 1) /= -1.0_c_double .or. sol(ldy, 2) /= -1.0_c_double) then
  print '(a)', 'a padding row was written'
  error stop 1
 end if
 sum_y = 0_c_int64_t
 sum_x = 0_c_int64_t
 do c = 1, n
  do i = 1, snps
   sum_y = ieor(sum_y, transfer(y(i, c), sum_y))
   sum_x = ieor(sum_x, transfer(sol(i, c), sum_x))
  end do
 end do
 print '(a,z16.16,a,z16.16,a,i0,1x,i0,a)', 'ld_op_check: apply ', sum_y, ' solve ', sum_x, ' iters ', iters(1), iters(2), ' PASS'
end program
