!==============================================================================
! md_simulation_gpu -- thin Fortran driver of the MI355X engine.
!
! Same inputs and outputs as the reference's production program for the part that touches
! the hot path (scripts/md_simulation_program.f90:208-391):
!   in : inputs/input_simulation_parameters.txt, outputs/rv_init.dat
!   out: outputs/one_run/instantaneous_energies.dat   header :294, rows :374
!        outputs/one_run/rva.dat                      header :254-257, records :384-387
!        outputs/one_run/corr_*.dat, corrmean_*.dat, md_final_results.txt   :401-560
!        (module md_stats / md_run_outputs: same estimators, same formats)
! Differences: the state lives in HBM for the whole run (ljmd_verlet_steps advances up to the
! next sampling step without touching the host; r, ru, v, a come back only when a snapshot is
! written) and the per-step unwrapped-coordinate update (:339-353) happens inside the drift
! kernel; snapshots leave the GPU through ljmd_snapshot_begin/end while the next steps already run.
! Environment: LJMD_DEVICE (default 0), LJMD_ASYNC_IO (default 1), LJMD_GPUS (default 1; > 1: this one process
! drives that many devices -- ljmd_create_multi, particles sharded by index range, RCCL all-gather of positions and
! reduce-scatter of forces per step inside the library -- e.g. BASELINE config 4 with LJMD_GPUS=8; LJMD_DEVICES, a
! comma-separated device list of that length, overrides 0..LJMD_GPUS-1), LJMD_REPRODUCIBLE (default 0; 1: the
! LJMD_PRECISION_FP64_REPRODUCIBLE mode -- every output file bitwise independent of LJMD_GPUS), LJMD_RDF_BINS
! (default 0 = off; > 0: g(r) with that many bins up to LJMD_RDF_RMAX, default half the box, is accumulated on the
! device -- ljmd_rdf_* -- at every sampling instant that writes an rva.dat record, over all particles, and
! outputs/one_run/rdf_gpu.dat gets the bin centres, integer counts and g(r), in the format of md_simulation_many_gpu;
! every other output file is the same with and without it), LJMD_TCF_MAX_LAG (default 0 = off; > 0: MSD(tau) and
! VACF(tau) of the resident system on the device -- ljmd_tcf_*, time-origin averaged over the same sampling instants,
! every LJMD_TCF_ORIGIN_STRIDE-th of them (default 1) an origin -- and outputs/one_run/msd_vacf_gpu.dat gets, per lag
! with at least one origin, lag, lag * output_interval * dt, the number of origins, MSD and VACF, in the format of
! md_simulation_many_gpu; one-rank engines only: with LJMD_GPUS > 1 the program stops before an engine is created;
! every other output file is the same with and without it), LJMD_STRESS (default 0 = off; 1: the pressure tensor of
! the resident system is recorded on the device -- ljmd_stress_* -- at the same sampling instants, with any LJMD_GPUS,
! and outputs/one_run/pressure_tensor_gpu.dat gets the time and p_xx, p_yy, p_zz, p_xy, p_xz, p_yz of every instant,
! without tail correction; with LJMD_STRESS_MAX_LAG > 0 outputs/one_run/stress_acf_gpu.dat also gets, per lag up to that
! many sampling instants, lag, tau, the time-origin averaged shear and normal-difference autocorrelations --
! ljmd_time_origin_average on the series as the velocity of one particle, each divided by its three components -- and the
! running Green-Kubo viscosities V / <T> times their trapezoid integrals; every other output file is the same with and
! without it), LJMD_HEATFLUX (default 0 = off; 1: the heat flux of the resident system is recorded on the device --
! ljmd_heatflux_* -- at the same sampling instants, and outputs/one_run/heat_flux_gpu.dat gets the time, J_x, J_y, J_z
! and the nine parts (convective, potential, collisional, x y z each) of every instant; with LJMD_HEATFLUX_MAX_LAG > 0
! outputs/one_run/heat_flux_acf_gpu.dat also gets, per lag up to that many sampling instants, lag, tau, the time-origin
! averaged <J(0) . J(tau)> / 3 -- ljmd_time_origin_average on the series as the velocity of one particle -- and the
! running Green-Kubo thermal conductivity V / <T>^2 times its trapezoid integral; one-rank engines only: with
! LJMD_GPUS > 1 the program stops before an engine is created; every other output file is the same with and without it),
! LJMD_VANHOVE_MAX_LAG (default 0 = off; > 0: the van Hove self-correlation of the resident system on the device --
! ljmd_vanhove_*, over the same sampling instants, every LJMD_VANHOVE_ORIGIN_STRIDE-th of them (default 1) an origin,
! LJMD_VANHOVE_BINS bins (default 128) up to LJMD_VANHOVE_RMAX (default half the box) -- and
! outputs/one_run/van_hove_gpu.dat gets, per lag with at least one origin, lag, tau, the number of origins, <r^2>, <r^4>,
! the non-Gaussian parameter, the overflow count and the row of counts; one-rank engines only: with LJMD_GPUS > 1 the
! program stops before an engine is created; every other output file is the same with and without it),
! LJMD_RHOK_N2MAX (default 0 = off; > 0: the collective density modes rho_k of the resident system are recorded on the
! device -- ljmd_rhok_* -- at the same sampling instants, for the modes ljmd_rhok_select_modes gives: the half-space
! triples with |n|^2 <= LJMD_RHOK_N2MAX, at most LJMD_RHOK_PER_SHELL (default 8) per shell of equal |n|^2;
! outputs/one_run/density_modes_gpu.dat gets a header line listing the modes and per instant the time, then Re and Im
! of every mode; outputs/one_run/structure_factor_gpu.dat per shell |n|^2, k, the number of modes and S(k) =
! <|rho_k|^2> / N; with LJMD_RHOK_MAX_LAG > 0 outputs/one_run/intermediate_scattering_gpu.dat also gets, per lag up to
! that many sampling instants, lag, tau and per shell the time-origin averaged F(k, tau) = <Re rho_k(t0 + tau)
! rho_k*(t0)> / N -- ljmd_time_origin_average with the shell's modes as the particles and (Re, Im, 0) as the velocity;
! one-rank engines only: with LJMD_GPUS > 1 the program stops before an engine is created; every other output file is
! the same with and without it),
! LJMD_CURRENT_N2MAX (default 0 = off; > 0: the collective current modes j_k of the resident system are recorded on the
! device -- ljmd_current_* -- at the same sampling instants, for the modes ljmd_rhok_select_modes gives with
! LJMD_CURRENT_N2MAX and LJMD_CURRENT_PER_SHELL (default 8), as LJMD_RHOK_N2MAX / PER_SHELL choose theirs;
! outputs/one_run/current_modes_gpu.dat gets a header line listing the modes and per instant the time, then Re and Im of
! the x, y and z component of every mode; outputs/one_run/current_correlations_gpu.dat per shell and lag |n|^2, k, lag,
! tau, C_L(k, tau) and C_T(k, tau): with LJMD_CURRENT_MAX_LAG > 0 and at least two instants the time-origin averages up
! to that many sampling instants -- ljmd_time_origin_average with the shell's modes as the particles, (Re j_L, Im j_L, 0)
! and the real and the imaginary part of j_T as the velocities -- otherwise lag 0 alone, the equal-time values over all
! instants; one-rank engines only: with LJMD_GPUS > 1 the program stops before an engine is created; every other output
! file is the same with and without it).
!==============================================================================
program md_simulation_gpu
  use, intrinsic :: iso_c_binding
  use define_precision, only: dp_kind, int_kind
  use md_types,         only: sim_params, sim_state, init_state
  use read_input_files, only: read_simulation_parameters
  use ljmd_c_api
  use lj_potential_energy, only: use_tail_corrections     ! the reference's compile-time switch (lj_potential_energy.f90:36)
  use md_stats,         only: run_statistics, stats_begin, stats_push, stats_mean_std, Q_T
  use md_run_outputs,   only: write_run_statistics, write_rdf_file, write_msd_vacf_file, write_pressure_tensor_file, &
                              write_stress_acf_file, write_heat_flux_file, write_heat_flux_acf_file, write_van_hove_file, &
                              write_density_modes_file, density_mode_shells, write_structure_factor_file, &
                              write_intermediate_scattering_file, write_current_modes_file, current_projections, &
                              current_equal_time, write_current_correlations_file
  implicit none

  type(sim_params) :: params
  type(sim_state), target :: state
  real(kind=dp_kind), allocatable, target :: rux(:), ruy(:), ruz(:)
  real(kind=dp_kind), allocatable, target :: s_epot(:), s_ekin(:), s_depot(:), s_ddepot(:)
  integer(kind=int_kind) :: total_steps, output_interval, warmup_steps, n_snapshots_expected
  real(kind=dp_kind) :: rc_over_L, target_total_energy
  real(kind=dp_kind) :: epot, ekin, etot, d_epot, dd_epot, time, temp_inst, press_inst, npd
  integer(kind=int_kind) :: step, count, k, num_samples
  logical :: sample_now, async_io, sampled_steps
  integer :: iu_rva, iu_out, ios, device, n_gpus
  integer(c_int32_t) :: precision_mode
  integer(c_int32_t), allocatable, target :: device_list(:)
  character(len=256) :: env_list
  integer(kind=8) :: c0, c1, crate
  type(c_ptr) :: engine
  type(run_statistics) :: stats
  character(len=32) :: env
  integer :: rdf_bins
  real(kind=dp_kind) :: rdf_rmax
  integer(c_int64_t), allocatable, target :: rdf_hist(:)
  integer(c_int64_t) :: rdf_snapshots
  integer :: tcf_max_lag, tcf_stride
  real(c_double), allocatable, target :: tcf_msd(:), tcf_vacf(:)           ! [tcf_max_lag + 1]
  integer(c_int64_t), allocatable, target :: tcf_counts(:)
  integer(c_int64_t) :: tcf_snapshots
  logical :: stress_on
  integer :: stress_max_lag, stress_lags
  real(c_double), allocatable, target :: stress_p(:, :), stress_times(:)   ! [6, snapshots], [snapshots]
  real(c_double), allocatable, target :: stress_c(:, :), stress_shear(:), stress_normal(:)
  integer(c_int64_t) :: stress_snapshots
  logical :: heatflux_on
  integer :: heatflux_max_lag, heatflux_lags
  real(c_double), allocatable, target :: heatflux_j(:, :), heatflux_parts(:, :, :)     ! [3, snapshots], [3, 3, snapshots]
  real(c_double), allocatable, target :: heatflux_times(:)
  real(c_double), allocatable, target :: heatflux_c(:, :), heatflux_acf(:)
  integer(c_int64_t) :: heatflux_snapshots
  real(kind=dp_kind) :: mean_temp, std_temp
  integer :: vh_max_lag, vh_stride, vh_bins
  real(kind=dp_kind) :: vh_rmax
  real(c_double), allocatable, target :: vh_r2(:), vh_r4(:)                ! [vh_max_lag + 1]
  integer(c_int64_t), allocatable, target :: vh_counts(:), vh_hist(:, :)   ! [vh_max_lag + 1], [vh_bins + 1, vh_max_lag + 1]
  integer(c_int64_t) :: vh_snapshots
  integer :: rhok_n2max, rhok_per_shell, rhok_max_lag, rhok_lags, rhok_shells, rhok_s, rhok_cnt
  integer(c_int32_t) :: rhok_n_modes
  integer(c_int) :: rhok_status
  integer(c_int32_t), allocatable, target :: rhok_modes(:, :)              ! [3, n_modes]
  integer, allocatable :: rhok_first(:)
  real(c_double), allocatable, target :: rhok_rho(:, :, :), rhok_times(:)  ! [2, n_modes, snapshots], [snapshots]
  real(c_double), allocatable, target :: rhok_re(:, :), rhok_im(:, :), rhok_zero(:, :), rhok_f(:, :), rhok_row(:)
  integer(c_int64_t) :: rhok_snapshots
  integer :: cur_n2max, cur_per_shell, cur_max_lag, cur_lags, cur_shells, cur_s, cur_cnt, cur_a, cur_first_shell
  integer(c_int32_t) :: cur_n_modes
  integer(c_int) :: cur_status
  integer(c_int32_t), allocatable, target :: cur_modes(:, :)               ! [3, n_modes]
  integer, allocatable :: cur_first(:)
  real(c_double), allocatable, target :: cur_j(:, :, :, :), cur_times(:)   ! [2, 3, n_modes, snapshots], [snapshots]
  real(c_double), allocatable :: cur_jl(:, :, :), cur_jt(:, :, :, :), cur_cl(:, :), cur_ct(:, :)
  real(c_double), allocatable, target :: cur_x(:, :), cur_y(:, :), cur_z(:, :), cur_row(:), cur_row2(:)
  integer(c_int64_t) :: cur_snapshots

  call read_simulation_parameters('inputs/input_simulation_parameters.txt', params, total_steps, &
                                  output_interval, warmup_steps, rc_over_L, target_total_energy)
  call init_state(params, state)
  call read_rv_init('outputs/rv_init.dat')
  allocate(rux(params%n), ruy(params%n), ruz(params%n))

  device = 0
  call get_environment_variable('LJMD_DEVICE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) device
  async_io = .true.
  call get_environment_variable('LJMD_ASYNC_IO', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) async_io = trim(env) /= '0'
  sampled_steps = .true.
  call get_environment_variable('LJMD_SAMPLED_STEPS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) sampled_steps = trim(env) /= '0'

  precision_mode = LJMD_PRECISION_FP64
  call get_environment_variable('LJMD_REPRODUCIBLE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) then
    if (trim(env) /= '0') precision_mode = LJMD_PRECISION_FP64_REPRODUCIBLE
  end if
  rdf_bins = 0
  call get_environment_variable('LJMD_RDF_BINS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rdf_bins
  if (rdf_bins < 0) stop 'md_simulation: LJMD_RDF_BINS must be >= 0.'
  rdf_rmax = 0.5d0 * params%box_length
  call get_environment_variable('LJMD_RDF_RMAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rdf_rmax
  tcf_max_lag = 0
  call get_environment_variable('LJMD_TCF_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) tcf_max_lag
  if (tcf_max_lag < 0) stop 'md_simulation: LJMD_TCF_MAX_LAG must be >= 0.'
  tcf_stride = 1
  call get_environment_variable('LJMD_TCF_ORIGIN_STRIDE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) tcf_stride
  if (tcf_stride < 1) stop 'md_simulation: LJMD_TCF_ORIGIN_STRIDE must be >= 1.'
  stress_on = .false.
  call get_environment_variable('LJMD_STRESS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) stress_on = trim(env) /= '0'
  stress_max_lag = 0
  call get_environment_variable('LJMD_STRESS_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) stress_max_lag
  if (stress_max_lag < 0) stop 'md_simulation: LJMD_STRESS_MAX_LAG must be >= 0.'
  heatflux_on = .false.
  call get_environment_variable('LJMD_HEATFLUX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) heatflux_on = trim(env) /= '0'
  heatflux_max_lag = 0
  call get_environment_variable('LJMD_HEATFLUX_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) heatflux_max_lag
  if (heatflux_max_lag < 0) stop 'md_simulation: LJMD_HEATFLUX_MAX_LAG must be >= 0.'
  vh_max_lag = 0
  call get_environment_variable('LJMD_VANHOVE_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_max_lag
  if (vh_max_lag < 0) stop 'md_simulation: LJMD_VANHOVE_MAX_LAG must be >= 0.'
  vh_stride = 1
  call get_environment_variable('LJMD_VANHOVE_ORIGIN_STRIDE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_stride
  if (vh_stride < 1) stop 'md_simulation: LJMD_VANHOVE_ORIGIN_STRIDE must be >= 1.'
  vh_bins = 128
  call get_environment_variable('LJMD_VANHOVE_BINS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_bins
  if (vh_bins < 1) stop 'md_simulation: LJMD_VANHOVE_BINS must be >= 1.'
  vh_rmax = 0.5d0 * params%box_length
  call get_environment_variable('LJMD_VANHOVE_RMAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_rmax
  rhok_n2max = 0
  call get_environment_variable('LJMD_RHOK_N2MAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_n2max
  if (rhok_n2max < 0) stop 'md_simulation: LJMD_RHOK_N2MAX must be >= 0.'
  rhok_per_shell = 8
  call get_environment_variable('LJMD_RHOK_PER_SHELL', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_per_shell
  if (rhok_per_shell < 1) stop 'md_simulation: LJMD_RHOK_PER_SHELL must be >= 1.'
  rhok_max_lag = 0
  call get_environment_variable('LJMD_RHOK_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_max_lag
  if (rhok_max_lag < 0) stop 'md_simulation: LJMD_RHOK_MAX_LAG must be >= 0.'
  cur_n2max = 0
  call get_environment_variable('LJMD_CURRENT_N2MAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) cur_n2max
  if (cur_n2max < 0) stop 'md_simulation: LJMD_CURRENT_N2MAX must be >= 0.'
  cur_per_shell = 8
  call get_environment_variable('LJMD_CURRENT_PER_SHELL', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) cur_per_shell
  if (cur_per_shell < 1) stop 'md_simulation: LJMD_CURRENT_PER_SHELL must be >= 1.'
  cur_max_lag = 0
  call get_environment_variable('LJMD_CURRENT_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) cur_max_lag
  if (cur_max_lag < 0) stop 'md_simulation: LJMD_CURRENT_MAX_LAG must be >= 0.'
  n_gpus = 1
  call get_environment_variable('LJMD_GPUS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) n_gpus
  if (n_gpus > 1 .and. tcf_max_lag > 0) &
    error stop 'md_simulation: LJMD_TCF_MAX_LAG needs a one-rank engine (n_ranks = 1): unset it or run with LJMD_GPUS=1.'
  if (n_gpus > 1 .and. heatflux_on) &
    error stop 'md_simulation: LJMD_HEATFLUX needs a one-rank engine (n_ranks = 1): unset it or run with LJMD_GPUS=1.'
  if (n_gpus > 1 .and. vh_max_lag > 0) &
    error stop 'md_simulation: LJMD_VANHOVE_MAX_LAG needs a one-rank engine (n_ranks = 1): unset it or run with LJMD_GPUS=1.'
  if (n_gpus > 1 .and. rhok_n2max > 0) &
    error stop 'md_simulation: LJMD_RHOK_N2MAX needs a one-rank engine (n_ranks = 1): unset it or run with LJMD_GPUS=1.'
  if (n_gpus > 1 .and. cur_n2max > 0) &
    error stop 'md_simulation: LJMD_CURRENT_N2MAX needs a one-rank engine (n_ranks = 1): unset it or run with LJMD_GPUS=1.'
  if (n_gpus > 1) then
    allocate(device_list(n_gpus))
    device_list = [(int(k - 1, c_int32_t), k = 1, n_gpus)]
    call get_environment_variable('LJMD_DEVICES', env_list, status=ios)
    if (ios == 0 .and. len_trim(env_list) > 0) read(env_list, *) device_list
    call ljmd_check(ljmd_create_multi(engine, params%n, params%box_length, params%dt, params%rc, &
                                      precision_mode, int(n_gpus, c_int32_t), c_loc(device_list)), &
                    c_null_ptr, 'ljmd_create_multi')
  else
    call ljmd_check(ljmd_create(engine, params%n, params%box_length, params%dt, params%rc, &
                                precision_mode, int(device, c_int32_t), 0_c_int32_t, 1_c_int32_t), &
                    c_null_ptr, 'ljmd_create')
  end if
  call ljmd_check(ljmd_set_tail_corrections(engine, merge(1_c_int32_t, 0_c_int32_t, use_tail_corrections)), engine, &
                  'ljmd_set_tail_corrections')
  ! H2D; the library sets ru <- r (md_simulation_program.f90:229-231)
  call ljmd_check(ljmd_set_state(engine, c_loc(state%rx), c_loc(state%ry), c_loc(state%rz), &
                                 c_loc(state%vx), c_loc(state%vy), c_loc(state%vz)), engine, 'ljmd_set_state')
  if (rdf_bins > 0) call ljmd_check(ljmd_rdf_configure(engine, int(rdf_bins, c_int32_t), rdf_rmax), engine, &
                                    'ljmd_rdf_configure')
  if (tcf_max_lag > 0) call ljmd_check(ljmd_tcf_configure(engine, int(tcf_max_lag, c_int32_t), int(tcf_stride, c_int32_t)), &
                                       engine, 'ljmd_tcf_configure')
  if (vh_max_lag > 0) call ljmd_check(ljmd_vanhove_configure(engine, int(vh_max_lag, c_int32_t), int(vh_stride, c_int32_t), &
                                                             int(vh_bins, c_int32_t), vh_rmax), engine, 'ljmd_vanhove_configure')
  if (stress_on) then
    n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
    if (n_snapshots_expected < 1) stop 'md_simulation: LJMD_STRESS needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_STRESS_MAX_SNAPSHOTS) stop 'md_simulation: more sampling instants than LJMD_STRESS_MAX_SNAPSHOTS.'
    call ljmd_check(ljmd_stress_configure(engine, int(n_snapshots_expected, c_int32_t)), engine, 'ljmd_stress_configure')
    allocate(stress_times(n_snapshots_expected))
  end if
  if (heatflux_on) then
    n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
    if (n_snapshots_expected < 1) stop 'md_simulation: LJMD_HEATFLUX needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_HEATFLUX_MAX_SNAPSHOTS) &
      stop 'md_simulation: more sampling instants than LJMD_HEATFLUX_MAX_SNAPSHOTS.'
    call ljmd_check(ljmd_heatflux_configure(engine, int(n_snapshots_expected, c_int32_t)), engine, 'ljmd_heatflux_configure')
    allocate(heatflux_times(n_snapshots_expected))
  end if
  if (rhok_n2max > 0) then
    n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
    if (n_snapshots_expected < 1) stop 'md_simulation: LJMD_RHOK_N2MAX needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_RHOK_MAX_SNAPSHOTS) stop 'md_simulation: more sampling instants than LJMD_RHOK_MAX_SNAPSHOTS.'
    ! the count first (the call fails by design: capacity 0), then the list
    rhok_status = ljmd_rhok_select_modes(int(rhok_n2max, c_int32_t), int(rhok_per_shell, c_int32_t), 0_c_int32_t, c_null_ptr, &
                                         rhok_n_modes)
    if (rhok_status == LJMD_OK .or. rhok_n_modes < 1) call ljmd_check(rhok_status, c_null_ptr, 'ljmd_rhok_select_modes')
    if (rhok_n_modes > LJMD_RHOK_MAX_MODES) stop 'md_simulation: more modes than LJMD_RHOK_MAX_MODES: lower LJMD_RHOK_N2MAX.'
    allocate(rhok_modes(3, rhok_n_modes))
    call ljmd_check(ljmd_rhok_select_modes(int(rhok_n2max, c_int32_t), int(rhok_per_shell, c_int32_t), rhok_n_modes, &
                                           c_loc(rhok_modes), rhok_n_modes), c_null_ptr, 'ljmd_rhok_select_modes')
    call ljmd_check(ljmd_rhok_configure(engine, rhok_n_modes, c_loc(rhok_modes), int(n_snapshots_expected, c_int32_t)), engine, &
                    'ljmd_rhok_configure')
    allocate(rhok_times(n_snapshots_expected))
  end if
  if (cur_n2max > 0) then
    n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
    if (n_snapshots_expected < 1) stop 'md_simulation: LJMD_CURRENT_N2MAX needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_CURRENT_MAX_SNAPSHOTS) &
      stop 'md_simulation: more sampling instants than LJMD_CURRENT_MAX_SNAPSHOTS.'
    ! the count first (the call fails by design: capacity 0), then the list
    cur_status = ljmd_rhok_select_modes(int(cur_n2max, c_int32_t), int(cur_per_shell, c_int32_t), 0_c_int32_t, c_null_ptr, &
                                        cur_n_modes)
    if (cur_status == LJMD_OK .or. cur_n_modes < 1) call ljmd_check(cur_status, c_null_ptr, 'ljmd_rhok_select_modes')
    if (cur_n_modes > LJMD_RHOK_MAX_MODES) stop 'md_simulation: more modes than LJMD_RHOK_MAX_MODES: lower LJMD_CURRENT_N2MAX.'
    allocate(cur_modes(3, cur_n_modes))
    call ljmd_check(ljmd_rhok_select_modes(int(cur_n2max, c_int32_t), int(cur_per_shell, c_int32_t), cur_n_modes, &
                                           c_loc(cur_modes), cur_n_modes), c_null_ptr, 'ljmd_rhok_select_modes')
    call ljmd_check(ljmd_current_configure(engine, cur_n_modes, c_loc(cur_modes), int(n_snapshots_expected, c_int32_t)), engine, &
                    'ljmd_current_configure')
    allocate(cur_times(n_snapshots_expected))
  end if
  ! t = 0 forces and energies (:236-243)
  call ljmd_check(ljmd_compute_forces(engine, epot, d_epot, dd_epot), engine, 'ljmd_compute_forces')
  call ljmd_check(ljmd_kinetic_energy(engine, ekin), engine, 'ljmd_kinetic_energy')
  etot = epot + ekin
  time = 0.d0

  open(newunit=iu_rva, file='outputs/one_run/rva.dat', form='unformatted', status='replace', &
       action='write', iostat=ios)
  if (ios /= 0) stop 'md_simulation: cannot open outputs/one_run/rva.dat'
  n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
  if (n_snapshots_expected < 0) n_snapshots_expected = 0
  write(iu_rva) params%n, params%box_length, params%dt, output_interval, n_snapshots_expected

  open(newunit=iu_out, file='outputs/one_run/instantaneous_energies.dat', status='replace', &
       action='write', iostat=ios)
  if (ios /= 0) stop 'md_simulation: cannot open outputs/one_run/instantaneous_energies.dat'
  write(iu_out, '(a)') '# time   epot   ekin   etot   T   P'

  allocate(s_epot(LJMD_MAX_PENDING_STEPS), s_ekin(LJMD_MAX_PENDING_STEPS), &
           s_depot(LJMD_MAX_PENDING_STEPS), s_ddepot(LJMD_MAX_PENDING_STEPS))
  npd = dble(params%n)
  call stats_begin(stats, params%n, params%volume, n_snapshots_expected)
  num_samples = 0
  step = 0
  call system_clock(c0, crate)
  ! Software pipeline: while the host formats and writes the sample taken at step s, the GPU is
  ! already running the steps up to the next sampling instant.  LJMD_ASYNC_IO=0 serialises the two
  ! (the next segment is enqueued only after the files are written) for A/B timing.
  count = segment_length(step)
  call enqueue_segment(count)
  do while (step < total_steps)
    call ljmd_check(ljmd_collect_steps(engine, count, c_loc(s_epot), c_loc(s_ekin), c_loc(s_depot), &
                                       c_loc(s_ddepot)), engine, 'ljmd_collect_steps')
    do k = 1, count
      time = time + params%dt                       ! accumulated as at :356
    end do
    step = step + count
    epot = s_epot(count); ekin = s_ekin(count); d_epot = s_depot(count); dd_epot = s_ddepot(count)
    etot = epot + ekin
    sample_now = step > warmup_steps .and. mod(step, output_interval) == 0       ! :361
    if (sample_now) call ljmd_check(ljmd_snapshot_begin(engine), engine, 'ljmd_snapshot_begin')
    ! g(r) of the same instant, on the device, ahead of the next segment in the engine's stream
    if (sample_now .and. rdf_bins > 0) call ljmd_check(ljmd_rdf_accumulate(engine), engine, 'ljmd_rdf_accumulate')
    if (sample_now .and. tcf_max_lag > 0) call ljmd_check(ljmd_tcf_accumulate(engine), engine, 'ljmd_tcf_accumulate')
    if (sample_now .and. vh_max_lag > 0) call ljmd_check(ljmd_vanhove_accumulate(engine), engine, 'ljmd_vanhove_accumulate')
    if (sample_now .and. stress_on) then
      call ljmd_check(ljmd_stress_accumulate(engine), engine, 'ljmd_stress_accumulate')
      stress_times(num_samples + 1) = time
    end if
    if (sample_now .and. heatflux_on) then
      call ljmd_check(ljmd_heatflux_accumulate(engine), engine, 'ljmd_heatflux_accumulate')
      heatflux_times(num_samples + 1) = time
    end if
    if (sample_now .and. rhok_n2max > 0) then
      call ljmd_check(ljmd_rhok_accumulate(engine), engine, 'ljmd_rhok_accumulate')
      rhok_times(num_samples + 1) = time
    end if
    if (sample_now .and. cur_n2max > 0) then
      call ljmd_check(ljmd_current_accumulate(engine), engine, 'ljmd_current_accumulate')
      cur_times(num_samples + 1) = time
    end if
    count = segment_length(step)
    if (async_io .and. count > 0) call enqueue_segment(count)
    if (sample_now) then
      num_samples = num_samples + 1
      call stats_push(stats, epot, ekin, d_epot, dd_epot, temp_inst, press_inst)   ! T, P as md_means.f90:221,227
      write(iu_out, '(1pe13.6,5(2x,1pe13.6))') time, epot, ekin, etot, temp_inst, press_inst
      call ljmd_check(ljmd_snapshot_end(engine, c_loc(state%rx), c_loc(state%ry), c_loc(state%rz), &
                                        c_loc(rux), c_loc(ruy), c_loc(ruz), &
                                        c_loc(state%vx), c_loc(state%vy), c_loc(state%vz), &
                                        c_loc(state%ax), c_loc(state%ay), c_loc(state%az)), engine, 'ljmd_snapshot_end')
      write(iu_rva) state%rx, state%ry, state%rz
      write(iu_rva) rux, ruy, ruz
      write(iu_rva) state%vx, state%vy, state%vz
      write(iu_rva) state%ax, state%ay, state%az
    end if
    if (.not. async_io .and. count > 0) call enqueue_segment(count)
  end do
  call system_clock(c1)
  close(iu_out)
  close(iu_rva)
  if (rdf_bins > 0) then
    allocate(rdf_hist(rdf_bins))
    call ljmd_check(ljmd_rdf_read(engine, c_loc(rdf_hist), rdf_snapshots), engine, 'ljmd_rdf_read')
  end if
  if (tcf_max_lag > 0) then
    allocate(tcf_msd(0:tcf_max_lag), tcf_vacf(0:tcf_max_lag), tcf_counts(0:tcf_max_lag))
    call ljmd_check(ljmd_tcf_read(engine, c_loc(tcf_msd), c_loc(tcf_vacf), c_loc(tcf_counts), tcf_snapshots), engine, &
                    'ljmd_tcf_read')
  end if
  if (vh_max_lag > 0) then
    allocate(vh_r2(0:vh_max_lag), vh_r4(0:vh_max_lag), vh_counts(0:vh_max_lag), vh_hist(0:vh_bins, 0:vh_max_lag))
    call ljmd_check(ljmd_vanhove_read(engine, c_loc(vh_hist), c_loc(vh_r2), c_loc(vh_r4), c_loc(vh_counts), vh_snapshots), &
                    engine, 'ljmd_vanhove_read')
  end if
  if (stress_on) then
    allocate(stress_p(6, max(num_samples, 1)))
    call ljmd_check(ljmd_stress_read(engine, c_loc(stress_p), stress_snapshots), engine, 'ljmd_stress_read')
    if (stress_snapshots /= num_samples) stop 'md_simulation: the pressure tensor series and the samples disagree.'
  end if
  if (heatflux_on) then
    allocate(heatflux_j(3, max(num_samples, 1)), heatflux_parts(3, 3, max(num_samples, 1)))
    call ljmd_check(ljmd_heatflux_read(engine, c_loc(heatflux_j), c_loc(heatflux_parts), heatflux_snapshots), engine, &
                    'ljmd_heatflux_read')
    if (heatflux_snapshots /= num_samples) stop 'md_simulation: the heat flux series and the samples disagree.'
  end if
  if (rhok_n2max > 0) then
    allocate(rhok_rho(2, rhok_n_modes, max(num_samples, 1)))
    call ljmd_check(ljmd_rhok_read(engine, c_loc(rhok_rho), rhok_snapshots), engine, 'ljmd_rhok_read')
    if (rhok_snapshots /= num_samples) stop 'md_simulation: the density mode series and the samples disagree.'
  end if
  if (cur_n2max > 0) then
    allocate(cur_j(2, 3, cur_n_modes, max(num_samples, 1)))
    call ljmd_check(ljmd_current_read(engine, c_loc(cur_j), cur_snapshots), engine, 'ljmd_current_read')
    if (cur_snapshots /= num_samples) stop 'md_simulation: the current mode series and the samples disagree.'
  end if
  call ljmd_destroy(engine)

  if (num_samples <= 0) stop 'md_simulation: no samples were taken (check warmup_steps/output_interval).'
  call write_run_statistics('outputs/one_run', params, total_steps, output_interval, warmup_steps, stats)
  if (rdf_bins > 0) call write_rdf_file('outputs/one_run/rdf_gpu.dat', params%n, params%box_length, rdf_rmax, rdf_bins, &
                                        rdf_hist, rdf_snapshots)
  if (tcf_max_lag > 0) call write_msd_vacf_file('outputs/one_run/msd_vacf_gpu.dat', tcf_max_lag, output_interval, params%dt, &
                                                tcf_counts, tcf_msd, tcf_vacf)
  if (vh_max_lag > 0) call write_van_hove_file('outputs/one_run/van_hove_gpu.dat', params%n, vh_max_lag, vh_bins, vh_rmax, &
                                               output_interval, params%dt, vh_counts, vh_r2, vh_r4, vh_hist)
  if (stress_on) then
    call write_pressure_tensor_file('outputs/one_run/pressure_tensor_gpu.dat', int(num_samples), stress_times, stress_p)
    if (stress_max_lag > 0 .and. num_samples >= 2) then
      ! the three shear components, then the three normal differences, as the velocity of one particle: [1, snapshots] each
      allocate(stress_c(num_samples, 6))
      stress_c(:, 1) = stress_p(4, 1:num_samples)
      stress_c(:, 2) = stress_p(5, 1:num_samples)
      stress_c(:, 3) = stress_p(6, 1:num_samples)
      stress_c(:, 4) = 0.5d0 * (stress_p(1, 1:num_samples) - stress_p(2, 1:num_samples))
      stress_c(:, 5) = 0.5d0 * (stress_p(2, 1:num_samples) - stress_p(3, 1:num_samples))
      stress_c(:, 6) = 0.5d0 * (stress_p(3, 1:num_samples) - stress_p(1, 1:num_samples))
      stress_lags = min(stress_max_lag, int(num_samples) - 1)
      allocate(stress_shear(0:stress_lags), stress_normal(0:stress_lags))
      call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), 1_c_int32_t, c_loc(stress_c(1, 1)), &
                                               c_loc(stress_c(1, 2)), c_loc(stress_c(1, 3)), int(stress_lags, c_int32_t), &
                                               1_c_int32_t, c_loc(stress_shear)), c_null_ptr, 'ljmd_time_origin_average')
      call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), 1_c_int32_t, c_loc(stress_c(1, 4)), &
                                               c_loc(stress_c(1, 5)), c_loc(stress_c(1, 6)), int(stress_lags, c_int32_t), &
                                               1_c_int32_t, c_loc(stress_normal)), c_null_ptr, 'ljmd_time_origin_average')
      stress_shear = stress_shear / 3.d0
      stress_normal = stress_normal / 3.d0
      call stats_mean_std(stats, Q_T, mean_temp, std_temp)
      call write_stress_acf_file('outputs/one_run/stress_acf_gpu.dat', stress_lags, output_interval, params%dt, params%volume, &
                                 mean_temp, stress_shear, stress_normal)
    end if
  end if
  if (heatflux_on) then
    call write_heat_flux_file('outputs/one_run/heat_flux_gpu.dat', int(num_samples), heatflux_times, heatflux_j, heatflux_parts)
    if (heatflux_max_lag > 0 .and. num_samples >= 2) then
      ! the three components as the velocity of one particle: [1, snapshots] each
      allocate(heatflux_c(num_samples, 3))
      heatflux_c(:, 1) = heatflux_j(1, 1:num_samples)
      heatflux_c(:, 2) = heatflux_j(2, 1:num_samples)
      heatflux_c(:, 3) = heatflux_j(3, 1:num_samples)
      heatflux_lags = min(heatflux_max_lag, int(num_samples) - 1)
      allocate(heatflux_acf(0:heatflux_lags))
      call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), 1_c_int32_t, c_loc(heatflux_c(1, 1)), &
                                               c_loc(heatflux_c(1, 2)), c_loc(heatflux_c(1, 3)), int(heatflux_lags, c_int32_t), &
                                               1_c_int32_t, c_loc(heatflux_acf)), c_null_ptr, 'ljmd_time_origin_average')
      heatflux_acf = heatflux_acf / 3.d0
      call stats_mean_std(stats, Q_T, mean_temp, std_temp)
      call write_heat_flux_acf_file('outputs/one_run/heat_flux_acf_gpu.dat', heatflux_lags, output_interval, params%dt, &
                                    params%volume, mean_temp, heatflux_acf)
    end if
  end if
  if (rhok_n2max > 0) then
    call write_density_modes_file('outputs/one_run/density_modes_gpu.dat', int(rhok_n_modes), rhok_modes, int(num_samples), &
                                  rhok_times, rhok_rho)
    call write_structure_factor_file('outputs/one_run/structure_factor_gpu.dat', params%n, params%box_length, int(rhok_n_modes), &
                                     rhok_modes, int(num_samples), rhok_rho)
    if (rhok_max_lag > 0 .and. num_samples >= 2) then
      ! per shell its modes as the particles and (Re, Im, 0) as the velocity: [modes of the shell, snapshots] each
      allocate(rhok_first(rhok_n_modes + 1))
      call density_mode_shells(int(rhok_n_modes), rhok_modes, rhok_shells, rhok_first)
      rhok_lags = min(rhok_max_lag, int(num_samples) - 1)
      allocate(rhok_f(0:rhok_lags, rhok_shells), rhok_row(0:rhok_lags))
      do rhok_s = 1, rhok_shells
        rhok_cnt = rhok_first(rhok_s + 1) - rhok_first(rhok_s)
        allocate(rhok_re(rhok_cnt, num_samples), rhok_im(rhok_cnt, num_samples), rhok_zero(rhok_cnt, num_samples))
        rhok_re = rhok_rho(1, rhok_first(rhok_s):rhok_first(rhok_s + 1) - 1, 1:num_samples)
        rhok_im = rhok_rho(2, rhok_first(rhok_s):rhok_first(rhok_s + 1) - 1, 1:num_samples)
        rhok_zero = 0.d0
        call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), int(rhok_cnt, c_int32_t), &
                                                 c_loc(rhok_re), c_loc(rhok_im), c_loc(rhok_zero), int(rhok_lags, c_int32_t), &
                                                 1_c_int32_t, c_loc(rhok_row)), c_null_ptr, 'ljmd_time_origin_average')
        rhok_f(:, rhok_s) = rhok_row / dble(params%n)
        deallocate(rhok_re, rhok_im, rhok_zero)
      end do
      call write_intermediate_scattering_file('outputs/one_run/intermediate_scattering_gpu.dat', rhok_shells, rhok_lags, &
                                              output_interval, params%dt, rhok_f)
    end if
  end if
  if (cur_n2max > 0) then
    call write_current_modes_file('outputs/one_run/current_modes_gpu.dat', int(cur_n_modes), cur_modes, int(num_samples), &
                                  cur_times, cur_j)
    allocate(cur_first(cur_n_modes + 1), cur_jl(2, cur_n_modes, num_samples), cur_jt(2, 3, cur_n_modes, num_samples))
    call density_mode_shells(int(cur_n_modes), cur_modes, cur_shells, cur_first)
    call current_projections(int(cur_n_modes), cur_modes, int(num_samples), cur_j, cur_jl, cur_jt)
    cur_first_shell = 1                 ! the list of ljmd_rhok_select_modes has no (0, 0, 0): every shell has a direction
    if (cur_max_lag > 0 .and. num_samples >= 2) then
      ! per shell its modes as the particles: (Re j_L, Im j_L, 0), then the real and the imaginary part of j_T
      cur_lags = min(cur_max_lag, int(num_samples) - 1)
      allocate(cur_cl(0:cur_lags, cur_shells), cur_ct(0:cur_lags, cur_shells), cur_row(0:cur_lags), cur_row2(0:cur_lags))
      do cur_s = 1, cur_shells
        cur_cnt = cur_first(cur_s + 1) - cur_first(cur_s)
        allocate(cur_x(cur_cnt, num_samples), cur_y(cur_cnt, num_samples), cur_z(cur_cnt, num_samples))
        cur_x = cur_jl(1, cur_first(cur_s):cur_first(cur_s + 1) - 1, 1:num_samples)
        cur_y = cur_jl(2, cur_first(cur_s):cur_first(cur_s + 1) - 1, 1:num_samples)
        cur_z = 0.d0
        call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), int(cur_cnt, c_int32_t), &
                                                 c_loc(cur_x), c_loc(cur_y), c_loc(cur_z), int(cur_lags, c_int32_t), &
                                                 1_c_int32_t, c_loc(cur_row)), c_null_ptr, 'ljmd_time_origin_average')
        cur_cl(:, cur_s) = cur_row / dble(params%n)
        cur_row2 = 0.d0
        do cur_a = 1, 2
          cur_x = cur_jt(cur_a, 1, cur_first(cur_s):cur_first(cur_s + 1) - 1, 1:num_samples)
          cur_y = cur_jt(cur_a, 2, cur_first(cur_s):cur_first(cur_s + 1) - 1, 1:num_samples)
          cur_z = cur_jt(cur_a, 3, cur_first(cur_s):cur_first(cur_s + 1) - 1, 1:num_samples)
          call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(num_samples, c_int32_t), int(cur_cnt, c_int32_t), &
                                                   c_loc(cur_x), c_loc(cur_y), c_loc(cur_z), int(cur_lags, c_int32_t), &
                                                   1_c_int32_t, c_loc(cur_row)), c_null_ptr, 'ljmd_time_origin_average')
          cur_row2 = cur_row2 + cur_row
        end do
        cur_ct(:, cur_s) = 0.5d0 * cur_row2 / dble(params%n)
        deallocate(cur_x, cur_y, cur_z)
      end do
    else
      cur_lags = 0
      allocate(cur_cl(0:0, cur_shells), cur_ct(0:0, cur_shells))
      call current_equal_time(params%n, int(cur_n_modes), int(num_samples), cur_jl, cur_jt, cur_shells, cur_first, &
                              cur_cl(0, :), cur_ct(0, :))
    end if
    call write_current_correlations_file('outputs/one_run/current_correlations_gpu.dat', params%box_length, int(cur_n_modes), &
                                         cur_modes, cur_shells, cur_first, cur_first_shell, cur_lags, output_interval, &
                                         params%dt, cur_cl, cur_ct)
  end if
  write(*, '(a,i0,a,i0,a,f10.2,a,es11.4,a)') 'md_simulation_gpu: N=', params%n, ' steps=', total_steps, &
    '  ', dble(total_steps) * dble(crate) / dble(max(c1 - c0, 1_8)), ' steps/s  ', &
    0.5d0 * npd * (npd - 1.d0) * dble(total_steps) * dble(crate) / dble(max(c1 - c0, 1_8)), ' pair-interactions/s'

contains

  ! Only the last step of a segment is read below (epot = s_epot(count) ...): the reference samples at :361 and
  ! nowhere else, so the steps in between run the forces-only pair kernel.  LJMD_SAMPLED_STEPS=0 evaluates the
  ! energy sums on every step as lj_potential_energy.f90 does (A/B timing; r, v, a are bit-identical either way).
  subroutine enqueue_segment(n_steps)
    integer(kind=int_kind), intent(in) :: n_steps
    if (sampled_steps) then
      call ljmd_check(ljmd_enqueue_steps_sampled(engine, n_steps), engine, 'ljmd_enqueue_steps_sampled')
    else
      call ljmd_check(ljmd_enqueue_steps(engine, n_steps), engine, 'ljmd_enqueue_steps')
    end if
  end subroutine

  ! steps from `from_step` to the next sampling instant of :361 (or to the end of the run), capped by
  ! the engine's pending-step limit; 0 when the run is complete
  function segment_length(from_step) result(n)
    integer(kind=int_kind), intent(in) :: from_step
    integer(kind=int_kind) :: n, nxt
    nxt = (from_step / output_interval + 1) * output_interval
    do while (nxt <= warmup_steps)
      nxt = nxt + output_interval
    end do
    nxt = min(nxt, total_steps)
    n = min(max(nxt - from_step, 0), LJMD_MAX_PENDING_STEPS)
  end function segment_length

  ! outputs/rv_init.dat: record 1 = rx ry rz, record 2 = vx vy vz (md_initial_config_program.f90:285-286)
  subroutine read_rv_init(filename)
    character(len=*), intent(in) :: filename
    integer :: iu, ierr
    open(newunit=iu, file=filename, form='unformatted', status='old', action='read', iostat=ierr)
    if (ierr /= 0) stop 'read_rv_init(): cannot open rv_init file.'
    read(iu) state%rx, state%ry, state%rz
    read(iu) state%vx, state%vy, state%vz
    close(iu)
  end subroutine read_rv_init

end program md_simulation_gpu
