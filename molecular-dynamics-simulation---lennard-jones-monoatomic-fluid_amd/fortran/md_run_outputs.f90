!==============================================================================
! md_run_outputs -- end-of-run files of a production run, in the reference's formats:
!   <dir>/corr_<obs>.dat, <dir>/corrmean_<obs>.dat   md_simulation_program.f90:419-526, :594-634
!   <dir>/md_final_results.txt (appended block)      md_simulation_program.f90:531-560
! <obs> = epot, ekin, etot, temp, press.  Used by md_simulation_gpu (samples from the GPU) and
! by md_stats_replay (samples from a file; CPU-only test of this module and md_stats).
!   <dir>/rdf_gpu.dat: the g(r) histogram a GPU driver accumulated on the device (write_rdf_file), shared by
!   md_simulation_gpu (ljmd_rdf_*) and md_simulation_many_gpu (ljmd_batch_rdf_*).
!   <dir>/msd_vacf_gpu.dat: MSD(tau) and VACF(tau) accumulated on the device (write_msd_vacf_file), shared by
!   md_simulation_gpu (ljmd_tcf_*) and md_simulation_many_gpu (ljmd_batch_tcf_*).
!   <dir>/pressure_tensor_gpu.dat, <dir>/stress_acf_gpu.dat: the pressure tensor md_simulation_gpu recorded on the device
!   (ljmd_stress_*) and its Green-Kubo autocorrelations (write_pressure_tensor_file, write_stress_acf_file).
!   <dir>/heat_flux_gpu.dat, <dir>/heat_flux_acf_gpu.dat: the heat flux md_simulation_gpu recorded on the device
!   (ljmd_heatflux_*) and its Green-Kubo autocorrelation (write_heat_flux_file, write_heat_flux_acf_file).
!   <dir>/van_hove_gpu.dat: the van Hove self-correlation md_simulation_gpu accumulated on the device (ljmd_vanhove_*):
!   per lag the moments, the non-Gaussian parameter and the counts of |displacement| (write_van_hove_file).
!   <dir>/density_modes_gpu.dat, <dir>/structure_factor_gpu.dat, <dir>/intermediate_scattering_gpu.dat: the density
!   modes rho_k md_simulation_gpu recorded on the device (ljmd_rhok_*), S(k) and F(k, tau) per shell of equal |n|^2
!   (write_density_modes_file, write_structure_factor_file, write_intermediate_scattering_file).
!   <dir>/current_modes_gpu.dat, <dir>/current_correlations_gpu.dat: the current modes j_k md_simulation_gpu recorded on
!   the device (ljmd_current_*) and C_L(k, tau), C_T(k, tau) per shell of equal |n|^2 (write_current_modes_file,
!   current_projections, current_equal_time, write_current_correlations_file).
!==============================================================================
module md_run_outputs
  use, intrinsic :: iso_c_binding, only: c_int64_t, c_int32_t
  use define_precision, only: dp_kind, int_kind
  use md_types,         only: sim_params
  use md_stats
  implicit none
  private
  public :: write_run_statistics, write_rdf_file, write_msd_vacf_file, write_pressure_tensor_file, write_stress_acf_file
  public :: write_heat_flux_file, write_heat_flux_acf_file, write_van_hove_file
  public :: write_density_modes_file, density_mode_shells, write_structure_factor_file, write_intermediate_scattering_file
  public :: write_current_modes_file, current_projections, current_equal_time, write_current_correlations_file

contains

  subroutine write_run_statistics(dir, params, total_steps, output_interval, warmup_steps, st)
    character(len=*), intent(in) :: dir
    type(sim_params), intent(in) :: params
    integer(kind=int_kind), intent(in) :: total_steps, output_interval, warmup_steps
    type(run_statistics), intent(in) :: st

    real(kind=dp_kind), allocatable :: c(:), cn(:)
    real(kind=dp_kind) :: mean(5), std(5)
    type(thermo_coefficients) :: tc
    integer(kind=int_kind) :: lag_max, n_blocks, k
    integer :: iu, ios

    if (st%n_samples <= 0) stop 'md_simulation: no samples were taken (check warmup_steps/output_interval).'

    ! the reference evaluates the coefficients (and may stop there) before it writes the curves
    call stats_thermo(st, tc)

    lag_max = stats_lag_limit(st%n_samples)
    if (lag_max >= 0) then
      if (size(st%series, 1) < st%n_samples) stop 'md_corr_add_sample(): series buffer is full.'
      allocate(c(0:lag_max), cn(0:lag_max))
      do k = 1, N_OBS
        call autocovariance(st%series(1:st%n_samples, k), lag_max, c)
        call normalise_by_lag0(lag_max, c, cn)
        call write_curve(dir // '/corr_' // trim(OBS_TAG(k)) // '.dat', '# lag   C(lag)   C_norm(lag)', &
                         'write_corr_file(): cannot open output file.', lag_max, c, cn)
      end do
      ! at most 5 blocks, each at least lag_max + 1 samples long (:475-478)
      n_blocks = min(5, st%n_samples / (lag_max + 1))
      if (n_blocks >= 1) then
        do k = 1, N_OBS
          call block_mean_autocovariance(st%series(1:st%n_samples, k), n_blocks, lag_max, c, cn)
          call write_curve(dir // '/corrmean_' // trim(OBS_TAG(k)) // '.dat', &
                           '# lag   <C(lag)>_blocks   <C_norm(lag)>_blocks', &
                           'write_corrmean_file(): cannot open output file.', lag_max, c, cn)
        end do
      end if
      deallocate(c, cn)
    end if

    do k = 1, 5            ! Q_U, Q_K, Q_E, Q_T, Q_P are quantities 1..5
      call stats_mean_std(st, k, mean(k), std(k))
    end do

    open(newunit=iu, file=dir // '/md_final_results.txt', access='append', action='write', iostat=ios)
    if (ios /= 0) stop 'md_simulation: cannot open outputs/one_run/md_final_results.txt'
    write(iu, '(a)') '************** MD PRODUCTION RESULTS **************'
    write(iu, '(a,1x,i8)')       'num_particles:', params%n
    write(iu, '(a,1x,i8)')       'num_cells:', params%num_cells
    write(iu, '(a,1x,1pe19.12)') 'box_length:', params%box_length
    write(iu, '(a,1x,1pe19.12)') 'volume:', params%volume
    write(iu, '(a,1x,1pe19.12)') 'density:', dble(params%n) / params%volume
    write(iu, '(a,1x,1pe19.12)') 'time_step:', params%dt
    write(iu, '(a,1x,i8)')       'output_interval:', output_interval
    write(iu, '(a,1x,i10)')      'total_steps:', total_steps
    write(iu, '(a,1x,i10)')      'warmup_steps:', warmup_steps
    write(iu, '(a)') '-------------------- Averages --------------------'
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') '<Epot>:', mean(Q_U), 'std:', std(Q_U)
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') '<Ekin>:', mean(Q_K), 'std:', std(Q_K)
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') '<Etot>:', mean(Q_E), 'std:', std(Q_E)
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') '<T>   :', mean(Q_T), 'std:', std(Q_T)
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') '<P>   :', mean(Q_P), 'std:', std(Q_P)
    write(iu, '(a)') '-------------- Thermodynamic coefficients --------------'
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'Temperature:', tc%temperature, 'Pressure:', tc%pressure
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'Ca_v:', tc%Ca_v, 'Ce_v:', tc%Ce_v
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'Ca_p:', tc%Ca_p, 'Ce_p:', tc%Ce_p
    ! three items on a two-item format: format reversion puts Gamma on its own line, as in the reference (:555)
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'kappa_S:', tc%K_S_inv, 'kappa_T:', tc%K_T_inv, 'Gamma:', tc%gamma
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'Alpha_E1:', tc%alpha_E1, 'Alpha_E2:', tc%alpha_E2
    write(iu, '(a,1x,1pe19.12,2x,a,1x,1pe19.12)') 'Alpha_S:', tc%alpha_S, 'Alpha_P:', tc%alpha_P
    write(iu, '(a)') '--------------------------------------------------------'
    write(iu, *)
    close(iu)
  end subroutine write_run_statistics

  ! rdf_gpu.dat: per bin its centre, the integer count (2 per unordered pair, summed over the snapshots) and
  ! g(r) = count / (snapshots N rho shell volume); bin edges k rmax / nbins, the last one rmax itself
  subroutine write_rdf_file(filename, n, box_length, rmax, nbins, hist, snapshots)
    character(len=*), intent(in) :: filename
    integer(kind=int_kind), intent(in) :: n
    real(kind=dp_kind), intent(in) :: box_length, rmax
    integer, intent(in) :: nbins
    integer(c_int64_t), intent(in) :: hist(nbins), snapshots
    real(kind=dp_kind), parameter :: pi = 3.141592653589793238462643383279502884d0
    real(kind=dp_kind) :: dr, e0, e1, rho, norm, g
    integer :: iu_rdf, ierr, kb
    dr = rmax / dble(nbins)
    rho = dble(n) / box_length**3
    open(newunit=iu_rdf, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_rdf_file(): cannot open rdf_gpu.dat.'
    write(iu_rdf, '(a)') '# r_center   count   g(r)'
    do kb = 1, nbins
      e0 = dble(kb - 1) * dr
      e1 = dble(kb) * dr
      if (kb == nbins) e1 = rmax
      norm = dble(snapshots) * dble(n) * rho * ((4.d0 / 3.d0) * pi * (e1**3 - e0**3))
      g = 0.d0
      if (norm > 0.d0) g = dble(hist(kb)) / norm
      write(iu_rdf, '(es24.16e3,2x,i0,2x,es24.16e3)') 0.5d0 * (e0 + e1), hist(kb), g
    end do
    close(iu_rdf)
  end subroutine write_rdf_file

  ! msd_vacf_gpu.dat: per lag with at least one origin, lag, tau = lag * output_interval * dt, the origins, MSD and VACF
  ! (ljmd_tcf_read / one run's column of ljmd_batch_tcf_read)
  subroutine write_msd_vacf_file(filename, max_lag, output_interval, dt, counts, msd, vacf)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: max_lag
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: dt
    integer(c_int64_t), intent(in) :: counts(0:max_lag)
    real(kind=dp_kind), intent(in) :: msd(0:max_lag), vacf(0:max_lag)
    integer :: iu_tcf, ierr, lag
    open(newunit=iu_tcf, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_msd_vacf_file(): cannot open msd_vacf_gpu.dat.'
    write(iu_tcf, '(a)') '# lag   tau   origins   MSD   VACF'
    do lag = 0, max_lag
      if (counts(lag) <= 0) cycle
      write(iu_tcf, '(i0,2x,es24.16e3,2x,i0,2(2x,es24.16e3))') lag, dble(lag) * dble(output_interval) * dt, &
        counts(lag), msd(lag), vacf(lag)
    end do
    close(iu_tcf)
  end subroutine write_msd_vacf_file

  ! van_hove_gpu.dat: a line with n, nbins, rmax and dr, then per lag with at least one origin: lag, tau = lag *
  ! output_interval * dt, the origins, <r^2>, <r^4>, alpha_2 = 3 <r^4> / (5 <r^2>^2) - 1 (0 where <r^2> = 0), the count
  ! of the overflow column (displacements of rmax and beyond) and the nbins counts of the bins [k dr, (k + 1) dr)
  ! (ljmd_vanhove_read; every row of counts sums, with its overflow, to n origins)
  subroutine write_van_hove_file(filename, n, max_lag, nbins, rmax, output_interval, dt, counts, r2, r4, hist)
    character(len=*), intent(in) :: filename
    integer(kind=int_kind), intent(in) :: n
    integer, intent(in) :: max_lag, nbins
    real(kind=dp_kind), intent(in) :: rmax
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: dt
    integer(c_int64_t), intent(in) :: counts(0:max_lag)
    real(kind=dp_kind), intent(in) :: r2(0:max_lag), r4(0:max_lag)
    integer(c_int64_t), intent(in) :: hist(0:nbins, 0:max_lag)
    real(kind=dp_kind) :: alpha2
    integer :: iu_vh, ierr, lag
    open(newunit=iu_vh, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_van_hove_file(): cannot open van_hove_gpu.dat.'
    write(iu_vh, '(a,i0,a,i0,2(a,es24.16e3))') '# n = ', n, '  nbins = ', nbins, '  rmax = ', rmax, '  dr = ', rmax / dble(nbins)
    write(iu_vh, '(a)') '# lag   tau   origins   <r^2>   <r^4>   alpha_2   overflow   counts[nbins]'
    do lag = 0, max_lag
      if (counts(lag) <= 0) cycle
      alpha2 = 0.d0
      if (r2(lag) /= 0.d0) alpha2 = (3.d0 * r4(lag)) / (5.d0 * (r2(lag) * r2(lag))) - 1.d0
      write(iu_vh, '(i0,2x,es24.16e3,2x,i0,3(2x,es24.16e3),*(2x,i0))') lag, dble(lag) * dble(output_interval) * dt, &
        counts(lag), r2(lag), r4(lag), alpha2, hist(nbins, lag), hist(0:nbins - 1, lag)
    end do
    close(iu_vh)
  end subroutine write_van_hove_file

  ! pressure_tensor_gpu.dat: per sampling instant its time and p_xx, p_yy, p_zz, p_xy, p_xz, p_yz (ljmd_stress_read: no
  ! tail correction); times(k) is the time of snapshot k
  subroutine write_pressure_tensor_file(filename, n_snapshots, times, p)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: n_snapshots
    real(kind=dp_kind), intent(in) :: times(n_snapshots), p(6, n_snapshots)
    integer :: iu_p, ierr, k
    open(newunit=iu_p, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_pressure_tensor_file(): cannot open pressure_tensor_gpu.dat.'
    write(iu_p, '(a)') '# time   p_xx   p_yy   p_zz   p_xy   p_xz   p_yz'
    do k = 1, n_snapshots
      write(iu_p, '(es24.16e3,6(2x,es24.16e3))') times(k), p(:, k)
    end do
    close(iu_p)
  end subroutine write_pressure_tensor_file

  ! stress_acf_gpu.dat: per lag, lag, tau = lag * output_interval * dt, the shear and the normal-difference
  ! autocorrelation (each a mean over three components) and the running Green-Kubo viscosity of each,
  ! eta(tau) = V / T * trapezoid integral of the ACF up to tau, with the run's mean temperature
  subroutine write_stress_acf_file(filename, max_lag, output_interval, dt, volume, temperature, shear, normal)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: max_lag
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: dt, volume, temperature
    real(kind=dp_kind), intent(in) :: shear(0:max_lag), normal(0:max_lag)
    real(kind=dp_kind) :: h, eta_s, eta_n
    integer :: iu_a, ierr, lag
    open(newunit=iu_a, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_stress_acf_file(): cannot open stress_acf_gpu.dat.'
    write(iu_a, '(a)') '# lag   tau   ACF_shear   ACF_normal   eta_shear   eta_normal'
    h = dble(output_interval) * dt
    eta_s = 0.d0
    eta_n = 0.d0
    do lag = 0, max_lag
      if (lag > 0) then
        eta_s = eta_s + 0.5d0 * (shear(lag) + shear(lag - 1)) * h
        eta_n = eta_n + 0.5d0 * (normal(lag) + normal(lag - 1)) * h
      end if
      write(iu_a, '(i0,5(2x,es24.16e3))') lag, dble(lag) * h, shear(lag), normal(lag), &
        (volume / temperature) * eta_s, (volume / temperature) * eta_n
    end do
    close(iu_a)
  end subroutine write_stress_acf_file

  ! heat_flux_gpu.dat: per sampling instant its time, J_x, J_y, J_z and the nine parts (ljmd_heatflux_read: convective
  ! x y z, potential x y z, collisional x y z, each over V); times(k) is the time of snapshot k
  subroutine write_heat_flux_file(filename, n_snapshots, times, j, parts)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: n_snapshots
    real(kind=dp_kind), intent(in) :: times(n_snapshots), j(3, n_snapshots), parts(3, 3, n_snapshots)
    integer :: iu_j, ierr, k
    open(newunit=iu_j, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_heat_flux_file(): cannot open heat_flux_gpu.dat.'
    write(iu_j, '(a)') '# time   J_x   J_y   J_z   conv_x   conv_y   conv_z   pot_x   pot_y   pot_z   coll_x   coll_y   coll_z'
    do k = 1, n_snapshots
      write(iu_j, '(es24.16e3,12(2x,es24.16e3))') times(k), j(:, k), parts(:, :, k)
    end do
    close(iu_j)
  end subroutine write_heat_flux_file

  ! heat_flux_acf_gpu.dat: per lag, lag, tau = lag * output_interval * dt, the autocorrelation <J(0) . J(tau)> / 3 and the
  ! running Green-Kubo thermal conductivity lambda(tau) = V / T^2 * trapezoid integral of the ACF up to tau, with the
  ! run's mean temperature (k_B = 1)
  subroutine write_heat_flux_acf_file(filename, max_lag, output_interval, dt, volume, temperature, acf)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: max_lag
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: dt, volume, temperature
    real(kind=dp_kind), intent(in) :: acf(0:max_lag)
    real(kind=dp_kind) :: h, run
    integer :: iu_a, ierr, lag
    open(newunit=iu_a, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_heat_flux_acf_file(): cannot open heat_flux_acf_gpu.dat.'
    write(iu_a, '(a)') '# lag   tau   ACF_J   lambda'
    h = dble(output_interval) * dt
    run = 0.d0
    do lag = 0, max_lag
      if (lag > 0) run = run + 0.5d0 * (acf(lag) + acf(lag - 1)) * h
      write(iu_a, '(i0,3(2x,es24.16e3))') lag, dble(lag) * h, acf(lag), (volume / (temperature * temperature)) * run
    end do
    close(iu_a)
  end subroutine write_heat_flux_acf_file

  ! density_modes_gpu.dat: a header line listing the modes (nx,ny,nz), then per sampling instant the time and Re, Im of
  ! rho_k of every mode in list order
  subroutine write_density_modes_file(filename, n_modes, modes, n_snapshots, times, rho)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: n_modes, n_snapshots
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    real(kind=dp_kind), intent(in) :: times(n_snapshots), rho(2, n_modes, n_snapshots)
    integer :: iu_r, ierr, k, m
    open(newunit=iu_r, file=filename, status='replace', action='write', recl=26 * (2 * n_modes + 1) + 64 + 24 * n_modes, &
         iostat=ierr)
    if (ierr /= 0) stop 'write_density_modes_file(): cannot open density_modes_gpu.dat.'
    write(iu_r, '(a)', advance='no') '# time   Re Im of rho_k, modes:'
    do m = 1, n_modes
      write(iu_r, '(a,i0,a,i0,a,i0,a)', advance='no') ' (', modes(1, m), ',', modes(2, m), ',', modes(3, m), ')'
    end do
    write(iu_r, '(a)') ''
    do k = 1, n_snapshots
      write(iu_r, '(es24.16e3)', advance='no') times(k)
      do m = 1, n_modes
        write(iu_r, '(2(2x,es24.16e3))', advance='no') rho(1, m, k), rho(2, m, k)
      end do
      write(iu_r, '(a)') ''
    end do
    close(iu_r)
  end subroutine write_density_modes_file

  ! the shells of a mode list grouped by |n|^2 (ljmd_rhok_select_modes): first(s) .. first(s + 1) - 1 are the modes of
  ! shell s; returns the number of shells
  subroutine density_mode_shells(n_modes, modes, n_shells, first)
    integer, intent(in) :: n_modes
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    integer, intent(out) :: n_shells, first(n_modes + 1)
    integer :: m, n2, prev
    n_shells = 0
    prev = -1
    do m = 1, n_modes
      n2 = int(modes(1, m))**2 + int(modes(2, m))**2 + int(modes(3, m))**2
      if (n2 /= prev) then
        n_shells = n_shells + 1
        first(n_shells) = m
        prev = n2
      end if
    end do
    first(n_shells + 1) = n_modes + 1
  end subroutine density_mode_shells

  ! structure_factor_gpu.dat: per shell |n|^2, k = 2 pi sqrt(|n|^2) / L, the number of modes and S(k) = <|rho_k|^2> / N
  ! over the snapshots and the shell's modes (per snapshot the mean over the modes, then the mean over the snapshots)
  subroutine write_structure_factor_file(filename, n, box_length, n_modes, modes, n_snapshots, rho)
    character(len=*), intent(in) :: filename
    integer(kind=int_kind), intent(in) :: n
    real(kind=dp_kind), intent(in) :: box_length
    integer, intent(in) :: n_modes, n_snapshots
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    real(kind=dp_kind), intent(in) :: rho(2, n_modes, n_snapshots)
    integer :: iu_s, ierr, s, m, k, n_shells, n2, cnt
    integer, allocatable :: first(:)
    real(kind=dp_kind) :: acc, snap
    real(kind=dp_kind), parameter :: two_pi = 6.283185307179586476925286766559d0
    allocate(first(n_modes + 1))
    call density_mode_shells(n_modes, modes, n_shells, first)
    open(newunit=iu_s, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_structure_factor_file(): cannot open structure_factor_gpu.dat.'
    write(iu_s, '(a)') '# n2   k   modes   S(k)'
    do s = 1, n_shells
      m = first(s)
      n2 = int(modes(1, m))**2 + int(modes(2, m))**2 + int(modes(3, m))**2
      cnt = first(s + 1) - first(s)
      acc = 0.d0
      do k = 1, n_snapshots
        snap = 0.d0
        do m = first(s), first(s + 1) - 1
          snap = snap + (rho(1, m, k) * rho(1, m, k) + rho(2, m, k) * rho(2, m, k))
        end do
        acc = acc + snap / dble(cnt) / dble(n)
      end do
      write(iu_s, '(i0,2x,es24.16e3,2x,i0,2x,es24.16e3)') n2, two_pi * sqrt(dble(n2)) / box_length, cnt, acc / dble(n_snapshots)
    end do
    close(iu_s)
  end subroutine write_structure_factor_file

  ! intermediate_scattering_gpu.dat: per lag, lag, tau = lag * output_interval * dt, then F(k, tau) of every shell
  subroutine write_intermediate_scattering_file(filename, n_shells, max_lag, output_interval, dt, f)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: n_shells, max_lag
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: dt
    real(kind=dp_kind), intent(in) :: f(0:max_lag, n_shells)
    integer :: iu_f, ierr, lag, s
    open(newunit=iu_f, file=filename, status='replace', action='write', recl=26 * (n_shells + 1) + 64, iostat=ierr)
    if (ierr /= 0) stop 'write_intermediate_scattering_file(): cannot open intermediate_scattering_gpu.dat.'
    write(iu_f, '(a)') '# lag   tau   F(k, tau) per shell, in the order of structure_factor_gpu.dat'
    do lag = 0, max_lag
      write(iu_f, '(i0,2x,es24.16e3)', advance='no') lag, dble(lag) * dble(output_interval) * dt
      do s = 1, n_shells
        write(iu_f, '(2x,es24.16e3)', advance='no') f(lag, s)
      end do
      write(iu_f, '(a)') ''
    end do
    close(iu_f)
  end subroutine write_intermediate_scattering_file

  ! current_modes_gpu.dat: a header line listing the modes (nx,ny,nz), then per sampling instant the time and, of every
  ! mode in list order, Re and Im of the x, the y and the z component of j_k
  subroutine write_current_modes_file(filename, n_modes, modes, n_snapshots, times, j)
    character(len=*), intent(in) :: filename
    integer, intent(in) :: n_modes, n_snapshots
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    real(kind=dp_kind), intent(in) :: times(n_snapshots), j(2, 3, n_modes, n_snapshots)
    integer :: iu_j, ierr, k, m
    open(newunit=iu_j, file=filename, status='replace', action='write', recl=26 * (6 * n_modes + 1) + 64 + 24 * n_modes, &
         iostat=ierr)
    if (ierr /= 0) stop 'write_current_modes_file(): cannot open current_modes_gpu.dat.'
    write(iu_j, '(a)', advance='no') '# time   Re Im of j_k x, y, z, modes:'
    do m = 1, n_modes
      write(iu_j, '(a,i0,a,i0,a,i0,a)', advance='no') ' (', modes(1, m), ',', modes(2, m), ',', modes(3, m), ')'
    end do
    write(iu_j, '(a)') ''
    do k = 1, n_snapshots
      write(iu_j, '(es24.16e3)', advance='no') times(k)
      do m = 1, n_modes
        write(iu_j, '(6(2x,es24.16e3))', advance='no') j(:, :, m, k)
      end do
      write(iu_j, '(a)') ''
    end do
    close(iu_j)
  end subroutine write_current_modes_file

  ! the longitudinal and transverse parts of a current series: k^ = n / |n|, j_L = k^ . j, j_T = j - k^ j_L, each in the
  ! order of analysis.current_correlations (products and sums over x, y, z in turn).  Modes with |n|^2 = 0 give zeros.
  subroutine current_projections(n_modes, modes, n_snapshots, j, j_l, j_t)
    integer, intent(in) :: n_modes, n_snapshots
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    real(kind=dp_kind), intent(in) :: j(2, 3, n_modes, n_snapshots)
    real(kind=dp_kind), intent(out) :: j_l(2, n_modes, n_snapshots), j_t(2, 3, n_modes, n_snapshots)
    integer :: k, m, a, c
    real(kind=dp_kind) :: nd(3), norm, khat(3)
    do m = 1, n_modes
      nd = dble(modes(:, m))
      norm = sqrt((nd(1) * nd(1) + nd(2) * nd(2)) + nd(3) * nd(3))
      khat = 0.d0
      if (norm > 0.d0) khat = nd / norm
      do k = 1, n_snapshots
        do c = 1, 2
          j_l(c, m, k) = (j(c, 1, m, k) * khat(1) + j(c, 2, m, k) * khat(2)) + j(c, 3, m, k) * khat(3)
          do a = 1, 3
            j_t(c, a, m, k) = j(c, a, m, k) - khat(a) * j_l(c, m, k)
          end do
        end do
      end do
    end do
  end subroutine current_projections

  ! the equal-time values per shell of |n|^2 > 0 (analysis.current_equal_time): C_L0 = <|j_L|^2> / N and C_T0 = 1/2
  ! <|j_T|^2> / N over the snapshots and the shell's modes (per snapshot the mean over the modes, then over the snapshots)
  subroutine current_equal_time(n, n_modes, n_snapshots, j_l, j_t, n_shells, first, c_l, c_t)
    integer(kind=int_kind), intent(in) :: n
    integer, intent(in) :: n_modes, n_snapshots, n_shells, first(n_modes + 1)
    real(kind=dp_kind), intent(in) :: j_l(2, n_modes, n_snapshots), j_t(2, 3, n_modes, n_snapshots)
    real(kind=dp_kind), intent(out) :: c_l(n_shells), c_t(n_shells)
    integer :: s, m, k, cnt
    real(kind=dp_kind) :: acc_l, acc_t, snap_l, snap_t
    do s = 1, n_shells
      cnt = first(s + 1) - first(s)
      acc_l = 0.d0
      acc_t = 0.d0
      do k = 1, n_snapshots
        snap_l = 0.d0
        snap_t = 0.d0
        do m = first(s), first(s + 1) - 1
          snap_l = snap_l + (j_l(1, m, k)**2 + j_l(2, m, k)**2) / dble(n)
          snap_t = snap_t + 0.5d0 * sum(j_t(1, :, m, k)**2 + j_t(2, :, m, k)**2) / dble(n)
        end do
        acc_l = acc_l + snap_l / dble(cnt)
        acc_t = acc_t + snap_t / dble(cnt)
      end do
      c_l(s) = acc_l / dble(n_snapshots)
      c_t(s) = acc_t / dble(n_snapshots)
    end do
  end subroutine current_equal_time

  ! current_correlations_gpu.dat: per shell of |n|^2 > 0 and per lag, |n|^2, k = 2 pi sqrt(|n|^2) / L, lag, tau = lag *
  ! output_interval * dt, C_L(k, tau) and C_T(k, tau); first_shell = the first shell of the mode list with |n|^2 > 0
  subroutine write_current_correlations_file(filename, box_length, n_modes, modes, n_shells, first, first_shell, max_lag, &
                                             output_interval, dt, c_l, c_t)
    character(len=*), intent(in) :: filename
    real(kind=dp_kind), intent(in) :: box_length, dt
    integer, intent(in) :: n_modes, n_shells, first(n_modes + 1), first_shell, max_lag
    integer(c_int32_t), intent(in) :: modes(3, n_modes)
    integer(kind=int_kind), intent(in) :: output_interval
    real(kind=dp_kind), intent(in) :: c_l(0:max_lag, n_shells), c_t(0:max_lag, n_shells)
    integer :: iu_c, ierr, s, m, n2, lag
    real(kind=dp_kind), parameter :: two_pi = 6.283185307179586476925286766559d0
    open(newunit=iu_c, file=filename, status='replace', action='write', iostat=ierr)
    if (ierr /= 0) stop 'write_current_correlations_file(): cannot open current_correlations_gpu.dat.'
    write(iu_c, '(a)') '# n2   k   lag   tau   C_L(k, tau)   C_T(k, tau)'
    do s = first_shell, n_shells
      m = first(s)
      n2 = int(modes(1, m))**2 + int(modes(2, m))**2 + int(modes(3, m))**2
      do lag = 0, max_lag
        write(iu_c, '(i0,2x,es24.16e3,2x,i0,3(2x,es24.16e3))') n2, two_pi * sqrt(dble(n2)) / box_length, lag, &
            dble(lag) * dble(output_interval) * dt, c_l(lag, s), c_t(lag, s)
      end do
    end do
    close(iu_c)
  end subroutine write_current_correlations_file

  subroutine write_curve(filename, header, errmsg, lag_max, c, cn)
    character(len=*), intent(in) :: filename, header, errmsg
    integer(kind=int_kind), intent(in) :: lag_max
    real(kind=dp_kind), intent(in) :: c(0:), cn(0:)
    integer :: iu, ios
    integer(kind=int_kind) :: lag
    open(newunit=iu, file=filename, status='replace', action='write', iostat=ios)
    if (ios /= 0) then
      write(*, '(a)') errmsg
      stop 1
    end if
    write(iu, '(a)') header
    do lag = 0, lag_max
      write(iu, '(i8,2(2x,1pe19.12))') lag, c(lag), cn(lag)
    end do
    close(iu)
  end subroutine write_curve

end module md_run_outputs
