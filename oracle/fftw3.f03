! fftw3.f03 -- TEST INFRASTRUCTURE ONLY.  The test oracle's own stand-in for FFTW 3's Fortran 2003 interface
! file, declaring just the names the reference's steps 2 and 3 use (src/cls_correlator.f90, src/cls_measurer.f90
! include this file inside a module that uses iso_c_binding).  The argument kinds are those FFTW documents for
! its legacy-free "new-array execute" interface; the bodies are the direct long-double DFT of oracle/ref_dft.c,
! not FFTW.
  integer(C_INT), parameter :: FFTW_ESTIMATE = 64

  interface
     type(C_PTR) function fftw_plan_dft_r2c_1d(n, in, out, flags) bind(C, name='fftw_plan_dft_r2c_1d')
       import
       integer(C_INT), value :: n
       real(C_DOUBLE), dimension(*), intent(out) :: in
       complex(C_DOUBLE_COMPLEX), dimension(*), intent(out) :: out
       integer(C_INT), value :: flags
     end function fftw_plan_dft_r2c_1d

     type(C_PTR) function fftw_plan_dft_c2r_1d(n, in, out, flags) bind(C, name='fftw_plan_dft_c2r_1d')
       import
       integer(C_INT), value :: n
       complex(C_DOUBLE_COMPLEX), dimension(*), intent(out) :: in
       real(C_DOUBLE), dimension(*), intent(out) :: out
       integer(C_INT), value :: flags
     end function fftw_plan_dft_c2r_1d

     subroutine fftw_execute_dft_r2c(p, in, out) bind(C, name='fftw_execute_dft_r2c')
       import
       type(C_PTR), value :: p
       real(C_DOUBLE), dimension(*), intent(inout) :: in
       complex(C_DOUBLE_COMPLEX), dimension(*), intent(out) :: out
     end subroutine fftw_execute_dft_r2c

     subroutine fftw_execute_dft_c2r(p, in, out) bind(C, name='fftw_execute_dft_c2r')
       import
       type(C_PTR), value :: p
       complex(C_DOUBLE_COMPLEX), dimension(*), intent(inout) :: in
       real(C_DOUBLE), dimension(*), intent(out) :: out
     end subroutine fftw_execute_dft_c2r
  end interface
