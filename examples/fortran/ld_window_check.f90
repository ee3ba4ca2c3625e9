! Windowed LD through the Fortran binding: mxa_ld_window_bounds and the eight device entries, each called once through modmiraculix_amd on raw binary
! inputs of the working directory, each result written as a raw binary file.  tests/test_fortran_ld_window_gpu.py compares the files bit for bit with the
! same entries called from Python -- the one check the interface blocks of the LD family have.
!
!   ld_window_check.out <snps> <indiv> <window> <max_dist>
! reads   plink.bin          snps rows of ceil(indiv / 4) bytes, PLINK coding, no missing code        (the plain entries)
!         plink_missing.bin  the same layout, with missing codes                                      (the _pairwise entries)
!         f.bin              snps doubles: allele frequencies
!         pos.bin, chrom.bin snps doubles / snps 32-bit integers: positions and chromosome codes
! writes  last.bin, rowptr.bin (32- / 64-bit integers), band.bin, scores.bin, band_pairwise.bin, scores_pairwise.bin (fixed window `window`, ldb = window + 1,
!         kind 0, adjust 1), rows.bin, wscores.bin, rows_pairwise.bin, wscores_pairwise.bin (the window `last`)
program ld_window_check
 use, intrinsic :: iso_c_binding
 use modmiraculix_amd
 implicit none
 integer(c_int) :: snps, indiv, window
 real(c_double) :: max_dist
 integer(c_long) :: bps, total, ldb
 integer(c_int8_t), allocatable, target :: plink(:), plink_missing(:)
 real(c_double), allocatable, target :: f(:), pos(:), band(:), scores(:), rows(:)
 integer(c_int), allocatable, target :: chrom(:), last(:)
 integer(c_long), allocatable, target :: rowptr(:)
 character(len=64) :: arg

 if (command_argument_count() < 4) then
  print '(a)', 'usage: ld_window_check.out <snps> <indiv> <window> <max_dist>'
  error stop 2
 end if
 call get_command_argument(1, arg); read(arg, *) snps
 call get_command_argument(2, arg); read(arg, *) indiv
 call get_command_argument(3, arg); read(arg, *) window
 call get_command_argument(4, arg); read(arg, *) max_dist
 bps = (int(indiv, c_long) + 3) / 4
 ldb = int(window, c_long) + 1
 allocate(plink(bps * snps), plink_missing(bps * snps), f(snps), pos(snps), chrom(snps), last(snps), rowptr(snps + 1), scores(snps))
 call read_i8('plink.bin', plink)
 call read_i8('plink_missing.bin', plink_missing)
 call read_f64('f.bin', f)
 call read_f64('pos.bin', pos)
 call read_i32('chrom.bin', chrom)

 ! the window by distance (host only)
 call check(mxa_ld_window_bounds(snps, c_loc(pos), c_loc(chrom), max_dist, -1_c_int, c_loc(last), c_loc(rowptr)), 'mxa_ld_window_bounds')
 call write_i32('last.bin', last)
 call write_i64('rowptr.bin', rowptr)
 total = rowptr(snps + 1)

 ! fixed window
 allocate(band(ldb * snps))
 call check(mxa_ld_band(c_loc(plink), snps, indiv, window, c_loc(band), ldb, 0_c_int, 1_c_int, c_loc(f)), 'mxa_ld_band')
 call write_f64('band.bin', band)
 call check(mxa_ld_scores(c_loc(plink), snps, indiv, window, c_loc(scores), 1_c_int, 1_c_int, c_loc(f)), 'mxa_ld_scores')
 call write_f64('scores.bin', scores)
 call check(mxa_ld_band_pairwise(c_loc(plink_missing), snps, indiv, window, c_loc(band), ldb, 0_c_int), 'mxa_ld_band_pairwise')
 call write_f64('band_pairwise.bin', band)
 call check(mxa_ld_scores_pairwise(c_loc(plink_missing), snps, indiv, window, c_loc(scores), 1_c_int), 'mxa_ld_scores_pairwise')
 call write_f64('scores_pairwise.bin', scores)

 ! the window `last`
 allocate(rows(total))
 call check(mxa_ld_window_rows(c_loc(plink), snps, indiv, c_loc(last), c_loc(rows), 0_c_int, 1_c_int, c_loc(f)), 'mxa_ld_window_rows')
 call write_f64('rows.bin', rows)
 call check(mxa_ld_window_scores(c_loc(plink), snps, indiv, c_loc(last), c_loc(scores), 1_c_int, 1_c_int, c_loc(f)), 'mxa_ld_window_scores')
 call write_f64('wscores.bin', scores)
 call check(mxa_ld_window_rows_pairwise(c_loc(plink_missing), snps, indiv, c_loc(last), c_loc(rows), 0_c_int), 'mxa_ld_window_rows_pairwise')
 call write_f64('rows_pairwise.bin', rows)
 call check(mxa_ld_window_scores_pairwise(c_loc(plink_missing), snps, indiv, c_loc(last), c_loc(scores), 1_c_int), 'mxa_ld_window_scores_pairwise')
 call write_f64('wscores_pairwise.bin', scores)
 print '(a,i0,a)', 'ld_window_check: ', total, ' stored entries, PASS'

contains
 subroutine check(rc, what)
  integer(c_int), intent(in) :: rc
  character(len=*), intent(in) :: what
  if (rc /= 0 .or. mxa_last_error() /= 0) then
   print '(a,a,i0,a,i0)', what, ' failed: rc ', rc, ', mxa_last_error ', mxa_last_error()
   error stop 1
  end if
 end subroutine

 subroutine read_i8(name, a)
  character(len=*), intent(in) :: name
  integer(c_int8_t), intent(out) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='old', action='read')
  read(un) a
  close(un)
 end subroutine
 subroutine read_i32(name, a)
  character(len=*), intent(in) :: name
  integer(c_int), intent(out) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='old', action='read')
  read(un) a
  close(un)
 end subroutine
 subroutine read_f64(name, a)
  character(len=*), intent(in) :: name
  real(c_double), intent(out) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='old', action='read')
  read(un) a
  close(un)
 end subroutine
 subroutine write_i32(name, a)
  character(len=*), intent(in) :: name
  integer(c_int), intent(in) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='replace', action='write')
  write(un) a
  close(un)
 end subroutine
 subroutine write_i64(name, a)
  character(len=*), intent(in) :: name
  integer(c_long), intent(in) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='replace', action='write')
  write(un) a
  close(un)
 end subroutine
 subroutine write_f64(name, a)
  character(len=*), intent(in) :: name
  real(c_double), intent(in) :: a(:)
  integer :: un
  open(newunit=un, file=name, access='stream', form='unformatted', status='replace', action='write')
  write(un) a
  close(un)
 end subroutine
end program
