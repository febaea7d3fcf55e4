!==============================================================================
! md_simulation_many_gpu -- the reference's run-many workflow (scripts/run_many_md_simuations/run_many_md.f90) on
! ONE batch handle of the MI355X engine (include/ljmd.h: ljmd_batch_*): all runs step together, one workgroup per run.
!
!   in : inputs/input_simulation_parameters.txt (as md_simulation_gpu)
!        outputs/run_NNNN/input_simulation_parameters.txt when it exists: that run takes k, dt, L and rc_over_L from
!        it (a state-point or size sweep in one batch handle, ljmd_batch_create_per_replica); its total_steps,
!        output_interval and warmup_steps must equal the shared file's, since all runs step in lockstep
!        outputs/run_NNNN/rv_init.dat when it exists, else the shared outputs/rv_init.dat -- with the shared file every
!        run is the same trajectory, as in the reference (run_many_md.f90:13-15 warns about it); callers who want
!        independent runs write one rv_init.dat per run (a run with its own N needs its own)
!   out: outputs/run_NNNN/ instantaneous_energies.dat, rva.dat, corr_*.dat, corrmean_*.dat, md_final_results.txt --
!        the files md_simulation_gpu writes into outputs/one_run/, same formats (module md_stats / md_run_outputs)
!        outputs/several_runs.txt -- the reference's two header lines, then one directory per run (run_many_md.f90:
!        30,48-49,74)
! Each run is the physics of md_simulation_gpu (the batch engine's contract, ljmd.h); the runs differ from it only by
! the summation order of the forces.  Every file of a run is byte-identical to what this program writes with
! LJMD_RUNS=1 and that run's parameters as the shared input.
! Environment: LJMD_RUNS (default 10, the reference's n_runs_default, run_many_md.f90:26), LJMD_DEVICE (default 0),
! LJMD_REPRODUCIBLE (default 0; 1: the batch handle runs in the LJMD_PRECISION_FP64_REPRODUCIBLE mode,
! ljmd_batch_set_precision -- every file of a run is then byte-identical to what md_simulation_gpu writes for that run
! with LJMD_REPRODUCIBLE=1), LJMD_RDF_BINS (default 0 = off; nbins > 0: g(r) of every run on the device,
! ljmd_batch_rdf_*: the pair-distance histogram up to L/2 of all particles is accumulated at every sampling instant that
! writes an rva.dat record, and outputs/run_NNNN/rdf_gpu.dat gets nbins lines of bin centre, integer count (2 per
! unordered pair) and g(r) with the reference's normalisation, scripts/md_one_run_analysis.py:586-594),
! LJMD_TCF_MAX_LAG (default 0 = off; > 0: MSD(tau) and VACF(tau) of every run on the device, ljmd_batch_tcf_*, time-origin
! averaged as compute_msd_tau_timeorig / compute_vacf_tau_timeorig, scripts/md_one_run_analysis.py:404-489, over the
! sampling instants that write an rva.dat record, every LJMD_TCF_ORIGIN_STRIDE-th of them (default 1) an origin;
! outputs/run_NNNN/msd_vacf_gpu.dat gets a header line and, per lag with at least one origin, lag, lag * output_interval *
! dt, the number of origins, MSD and VACF),
! LJMD_STRESS (default 0 = off; 1: the pressure tensor of every run is recorded on the device, ljmd_batch_stress_*, at
! every sampling instant that writes an rva.dat record; outputs/run_NNNN/pressure_tensor_gpu.dat gets per instant its time
! and p_xx, p_yy, p_zz, p_xy, p_xz, p_yz without tail correction, and with LJMD_STRESS_MAX_LAG > 0
! outputs/run_NNNN/stress_acf_gpu.dat the shear and normal-difference autocorrelations and running Green-Kubo
! viscosities of the run -- the files and formats of md_simulation_gpu; every other file stays byte-identical),
! LJMD_HEATFLUX (default 0 = off; 1: the heat flux of every run is recorded on the device, ljmd_batch_heatflux_*, at every
! sampling instant that writes an rva.dat record; outputs/run_NNNN/heat_flux_gpu.dat gets per instant its time, J_x, J_y,
! J_z and the nine parts, and with LJMD_HEATFLUX_MAX_LAG > 0 outputs/run_NNNN/heat_flux_acf_gpu.dat the autocorrelation
! and running Green-Kubo thermal conductivity of the run -- the files and formats of md_simulation_gpu; every other file
! stays byte-identical),
! LJMD_VANHOVE_MAX_LAG (default 0 = off; > 0: the van Hove self-correlation of every run on the device,
! ljmd_batch_vanhove_*, over the sampling instants that write an rva.dat record -- those of MSD / VACF -- every
! LJMD_VANHOVE_ORIGIN_STRIDE-th of them (default 1) an origin, LJMD_VANHOVE_BINS bins (default 128) up to
! LJMD_VANHOVE_RMAX (default half of each run's box); outputs/run_NNNN/van_hove_gpu.dat is the file of md_simulation_gpu
! (md_run_outputs: write_van_hove_file); every other file stays byte-identical),
! LJMD_RHOK_N2MAX (default 0 = off; > 0: the collective density modes rho_k of every run are recorded on the device,
! ljmd_batch_rhok_*, at every sampling instant that writes an rva.dat record, for the one mode list
! ljmd_rhok_select_modes gives: the half-space triples with |n|^2 <= LJMD_RHOK_N2MAX, at most LJMD_RHOK_PER_SHELL
! (default 8) per shell, k = 2 pi n / L of the run's own box; outputs/run_NNNN/density_modes_gpu.dat and
! structure_factor_gpu.dat and, with LJMD_RHOK_MAX_LAG > 0, intermediate_scattering_gpu.dat are the files of
! md_simulation_gpu (md_run_outputs: write_density_modes_file, write_structure_factor_file,
! write_intermediate_scattering_file); every other file stays byte-identical),
! LJMD_SEED_BASE (unset: the rv_init.dat files above are read; s >= 1: NO rv_init.dat is read -- run i is prepared on the
! device, ljmd_batch_prepare, with seed s + i - 1: the reference's FCC lattice, its generator's velocities, centre of
! mass removed, scaled to the target_total_energy of the run's own or the shared input file, then that file's
! warmup_steps Verlet steps, as md_initial_config_gpu prepares one system with the seed 12345; the prepared state is
! written to outputs/run_NNNN/rv_init_gpu.dat in the rv_init.dat format -- the user's own rv_init.dat files are left
! alone -- and the production loop follows unchanged.  The runs are then independent trajectories; run i is
! byte-identical to LJMD_RUNS=1 with LJMD_SEED_BASE = s + i - 1 and that run's parameters).
! Batches take n <= LJMD_BATCH_MAX_N.
!==============================================================================
program md_simulation_many_gpu
  use, intrinsic :: iso_c_binding
  use define_precision, only: dp_kind, int_kind
  use md_types,         only: sim_params
  use read_input_files, only: read_simulation_parameters
  use ljmd_c_api
  use lj_potential_energy, only: use_tail_corrections     ! the reference's compile-time switch (lj_potential_energy.f90:36)
  use md_stats,         only: run_statistics, stats_begin, stats_push, stats_mean_std, Q_T
  use md_run_outputs,   only: write_run_statistics, write_rdf_file, write_msd_vacf_file, write_pressure_tensor_file, &
                              write_stress_acf_file, write_heat_flux_file, write_heat_flux_acf_file, write_van_hove_file, &
                              write_density_modes_file, write_structure_factor_file, write_intermediate_scattering_file, &
                              density_mode_shells
  implicit none

  character(len=*), parameter :: runs_list = 'outputs/several_runs.txt'
  type(sim_params) :: params
  type(sim_params), allocatable :: rparams(:)       ! each run's parameters: its own file's or the shared ones
  logical, allocatable :: own_params(:)
  integer(kind=8), allocatable :: off(:)            ! run i's particles: elements off(i) + 1 .. off(i + 1)
  integer(c_int32_t), allocatable :: n_c(:)
  real(c_double), allocatable :: box_c(:), dt_c(:), rc_c(:), time_run(:)
  integer :: seed_base                              ! LJMD_SEED_BASE, 0: unset
  integer(c_int32_t), allocatable, target :: seeds_c(:)
  real(c_double), allocatable, target :: target_run(:)     ! each run's target_total_energy: its own file's or the shared one
  logical :: any_own
  integer(kind=int_kind) :: total_steps, output_interval, warmup_steps, n_snapshots_expected
  real(kind=dp_kind) :: rc_over_L, target_total_energy
  real(kind=dp_kind), allocatable, target :: rx(:), ry(:), rz(:), ux(:), uy(:), uz(:)
  real(kind=dp_kind), allocatable, target :: vx(:), vy(:), vz(:), ax(:), ay(:), az(:)
  real(kind=dp_kind), allocatable, target :: s_epot(:), s_ekin(:), s_depot(:), s_ddepot(:)
  type(run_statistics), allocatable :: stats(:)
  integer, allocatable :: iu_rva(:), iu_out(:)
  character(len=64), allocatable :: run_dir(:)
  real(kind=dp_kind) :: time, etot, temp_inst, press_inst
  integer(kind=int_kind) :: step, k, num_samples, n, ni, rest
  integer :: n_runs, i, ios, device, iu
  integer(c_int32_t) :: n_runs_c, precision_mode
  integer(kind=8) :: c0, c1, crate, o, total
  type(c_ptr) :: batch
  character(len=32) :: env
  integer :: rdf_bins
  integer(c_int64_t), allocatable, target :: rdf_hist(:, :)     ! [rdf_bins, n_runs]
  integer(c_int64_t) :: rdf_snapshots
  integer :: tcf_max_lag, tcf_stride
  real(c_double), allocatable, target :: tcf_msd(:, :), tcf_vacf(:, :)     ! [tcf_max_lag + 1, n_runs]
  integer(c_int64_t), allocatable, target :: tcf_counts(:)
  integer(c_int64_t) :: tcf_snapshots
  logical :: stress_on
  integer :: stress_max_lag
  real(c_double), allocatable, target :: stress_p(:, :, :)      ! [6, n_runs, snapshots]
  real(c_double), allocatable :: stress_times(:, :)             ! [snapshots, n_runs]
  integer(c_int64_t) :: stress_snapshots
  logical :: heatflux_on
  integer :: heatflux_max_lag
  real(c_double), allocatable, target :: heatflux_j(:, :, :), heatflux_parts(:, :, :, :)   ! [3, n_runs, snapshots], [3, 3, ...]
  real(c_double), allocatable :: heatflux_times(:, :)           ! [snapshots, n_runs]
  integer(c_int64_t) :: heatflux_snapshots
  integer :: vh_max_lag, vh_stride, vh_bins
  logical :: vh_rmax_given
  real(kind=dp_kind) :: vh_rmax_env
  real(c_double), allocatable, target :: vh_rmax(:)                         ! [n_runs]
  real(c_double), allocatable, target :: vh_r2(:, :), vh_r4(:, :)           ! [vh_max_lag + 1, n_runs]
  integer(c_int64_t), allocatable, target :: vh_counts(:), vh_hist(:, :, :) ! [vh_max_lag + 1], [vh_bins + 1, vh_max_lag + 1, n_runs]
  integer(c_int64_t) :: vh_snapshots
  integer :: rhok_n2max, rhok_per_shell, rhok_max_lag
  integer(c_int32_t) :: rhok_n_modes
  integer(c_int) :: rhok_status
  integer(c_int32_t), allocatable, target :: rhok_modes(:, :)              ! [3, n_modes]
  real(c_double), allocatable, target :: rhok_rho(:, :, :, :)              ! [2, n_modes, n_runs, snapshots]
  real(c_double), allocatable :: rhok_times(:, :)                          ! [snapshots, n_runs]
  integer(c_int64_t) :: rhok_snapshots

  call read_simulation_parameters('inputs/input_simulation_parameters.txt', params, total_steps, &
                                  output_interval, warmup_steps, rc_over_L, target_total_energy)
  n = params%n
  n_runs = 10
  call get_environment_variable('LJMD_RUNS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) n_runs
  if (n_runs < 1) stop 'md_simulation_many: LJMD_RUNS must be >= 1.'
  device = 0
  call get_environment_variable('LJMD_DEVICE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) device
  precision_mode = LJMD_PRECISION_FP64
  call get_environment_variable('LJMD_REPRODUCIBLE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) then
    if (trim(env) /= '0') precision_mode = LJMD_PRECISION_FP64_REPRODUCIBLE
  end if
  rdf_bins = 0
  call get_environment_variable('LJMD_RDF_BINS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rdf_bins
  if (rdf_bins < 0) stop 'md_simulation_many: LJMD_RDF_BINS must be >= 0.'
  tcf_max_lag = 0
  call get_environment_variable('LJMD_TCF_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) tcf_max_lag
  if (tcf_max_lag < 0) stop 'md_simulation_many: LJMD_TCF_MAX_LAG must be >= 0.'
  tcf_stride = 1
  call get_environment_variable('LJMD_TCF_ORIGIN_STRIDE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) tcf_stride
  if (tcf_stride < 1) stop 'md_simulation_many: LJMD_TCF_ORIGIN_STRIDE must be >= 1.'
  stress_on = .false.
  call get_environment_variable('LJMD_STRESS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) stress_on = trim(env) /= '0'
  stress_max_lag = 0
  call get_environment_variable('LJMD_STRESS_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) stress_max_lag
  if (stress_max_lag < 0) stop 'md_simulation_many: LJMD_STRESS_MAX_LAG must be >= 0.'
  heatflux_on = .false.
  call get_environment_variable('LJMD_HEATFLUX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) heatflux_on = trim(env) /= '0'
  heatflux_max_lag = 0
  call get_environment_variable('LJMD_HEATFLUX_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) heatflux_max_lag
  if (heatflux_max_lag < 0) stop 'md_simulation_many: LJMD_HEATFLUX_MAX_LAG must be >= 0.'
  vh_max_lag = 0
  call get_environment_variable('LJMD_VANHOVE_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_max_lag
  if (vh_max_lag < 0) stop 'md_simulation_many: LJMD_VANHOVE_MAX_LAG must be >= 0.'
  vh_stride = 1
  call get_environment_variable('LJMD_VANHOVE_ORIGIN_STRIDE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_stride
  if (vh_stride < 1) stop 'md_simulation_many: LJMD_VANHOVE_ORIGIN_STRIDE must be >= 1.'
  vh_bins = 128
  call get_environment_variable('LJMD_VANHOVE_BINS', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) vh_bins
  if (vh_bins < 1) stop 'md_simulation_many: LJMD_VANHOVE_BINS must be >= 1.'
  vh_rmax_given = .false.
  vh_rmax_env = 0.d0
  call get_environment_variable('LJMD_VANHOVE_RMAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) then
    read(env, *) vh_rmax_env
    vh_rmax_given = .true.
  end if
  rhok_n2max = 0
  call get_environment_variable('LJMD_RHOK_N2MAX', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_n2max
  if (rhok_n2max < 0) stop 'md_simulation_many: LJMD_RHOK_N2MAX must be >= 0.'
  rhok_per_shell = 8
  call get_environment_variable('LJMD_RHOK_PER_SHELL', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_per_shell
  if (rhok_per_shell < 1) stop 'md_simulation_many: LJMD_RHOK_PER_SHELL must be >= 1.'
  rhok_max_lag = 0
  call get_environment_variable('LJMD_RHOK_MAX_LAG', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) read(env, *) rhok_max_lag
  if (rhok_max_lag < 0) stop 'md_simulation_many: LJMD_RHOK_MAX_LAG must be >= 0.'

  seed_base = 0
  call get_environment_variable('LJMD_SEED_BASE', env, status=ios)
  if (ios == 0 .and. len_trim(env) > 0) then
    read(env, *) seed_base
    if (seed_base < 1) stop 'md_simulation_many: LJMD_SEED_BASE must be >= 1.'
    if (seed_base > huge(1_c_int32_t) - (n_runs - 1)) stop 'md_simulation_many: LJMD_SEED_BASE + LJMD_RUNS - 1 exceeds int32.'
  end if

  allocate(rparams(n_runs), own_params(n_runs), off(n_runs + 1), time_run(n_runs), target_run(n_runs))
  allocate(s_epot(n_runs), s_ekin(n_runs), s_depot(n_runs), s_ddepot(n_runs))
  allocate(stats(n_runs), iu_rva(n_runs), iu_out(n_runs), run_dir(n_runs))

  ! run directories and parameters (before the GPU is touched); the runs' particles one after another
  off(1) = 0
  do i = 1, n_runs
    write(run_dir(i), '(a,i4.4)') 'outputs/run_', i
    call execute_command_line('mkdir -p ' // trim(run_dir(i)), exitstat=ios)
    if (ios /= 0) stop 'md_simulation_many: cannot create a run directory under outputs/.'
    call read_run_parameters(i)
    off(i + 1) = off(i) + rparams(i)%n
  end do
  any_own = any(own_params)
  total = off(n_runs + 1)
  allocate(rx(total), ry(total), rz(total), ux(total), uy(total), uz(total), &
           vx(total), vy(total), vz(total), ax(total), ay(total), az(total))
  if (seed_base == 0) then
    do i = 1, n_runs
      call read_rv_init(i)
    end do
  end if

  if (any_own) then
    allocate(n_c(n_runs), box_c(n_runs), dt_c(n_runs), rc_c(n_runs))
    do i = 1, n_runs
      n_c(i) = int(rparams(i)%n, c_int32_t)
      box_c(i) = rparams(i)%box_length
      dt_c(i) = rparams(i)%dt
      rc_c(i) = rparams(i)%rc
    end do
    call ljmd_batch_check(ljmd_batch_create_per_replica(batch, int(n_runs, c_int32_t), n_c, box_c, dt_c, rc_c, &
                                                        LJMD_PRECISION_FP64, int(device, c_int32_t)), c_null_ptr, &
                          'ljmd_batch_create_per_replica')
  else
    call ljmd_batch_check(ljmd_batch_create(batch, int(n_runs, c_int32_t), n, params%box_length, params%dt, params%rc, &
                                            LJMD_PRECISION_FP64, int(device, c_int32_t)), c_null_ptr, 'ljmd_batch_create')
  end if
  n_runs_c = int(n_runs, c_int32_t)
  ! a new batch handle is fp64 (the creators take no other mode); the mode is set before the state
  call ljmd_batch_check(ljmd_batch_set_precision(batch, precision_mode), batch, 'ljmd_batch_set_precision')
  call ljmd_batch_check(ljmd_batch_set_tail_corrections(batch, merge(1_c_int32_t, 0_c_int32_t, use_tail_corrections)), &
                        batch, 'ljmd_batch_set_tail_corrections')
  if (seed_base == 0) then
    ! H2D; the library sets ru <- r (md_simulation_program.f90:229-231)
    call ljmd_batch_check(ljmd_batch_set_state(batch, c_loc(rx), c_loc(ry), c_loc(rz), c_loc(vx), c_loc(vy), &
                                               c_loc(vz)), batch, 'ljmd_batch_set_state')
  else
    call prepare_on_device()
  end if
  if (rdf_bins > 0) call ljmd_batch_check(ljmd_batch_rdf_configure(batch, int(rdf_bins, c_int32_t), c_null_ptr, &
                                                                   0_c_int32_t), batch, 'ljmd_batch_rdf_configure')
  if (tcf_max_lag > 0) call ljmd_batch_check(ljmd_batch_tcf_configure(batch, int(tcf_max_lag, c_int32_t), &
                                                                      int(tcf_stride, c_int32_t), 0_c_int32_t), batch, &
                                             'ljmd_batch_tcf_configure')
  if (vh_max_lag > 0) then
    allocate(vh_rmax(n_runs))
    do i = 1, n_runs
      vh_rmax(i) = merge(vh_rmax_env, 0.5d0 * rparams(i)%box_length, vh_rmax_given)
    end do
    call ljmd_batch_check(ljmd_batch_vanhove_configure(batch, int(vh_max_lag, c_int32_t), int(vh_stride, c_int32_t), &
                                                       int(vh_bins, c_int32_t), c_loc(vh_rmax), 0_c_int32_t), batch, &
                          'ljmd_batch_vanhove_configure')
  end if
  ! t = 0 forces and energies of every run (:236-243)
  call ljmd_batch_check(ljmd_batch_compute_forces(batch, c_loc(s_epot), c_loc(s_depot), c_loc(s_ddepot)), batch, &
                        'ljmd_batch_compute_forces')
  call ljmd_batch_check(ljmd_batch_kinetic_energy(batch, c_loc(s_ekin)), batch, 'ljmd_batch_kinetic_energy')
  time_run = 0.d0

  n_snapshots_expected = (total_steps / output_interval) - (warmup_steps / output_interval)
  if (n_snapshots_expected < 0) n_snapshots_expected = 0
  if (stress_on) then
    ! one snapshot per sampling instant that writes an rva.dat record, taken by hand as g(r) and MSD / VACF are
    if (n_snapshots_expected < 1) stop 'md_simulation_many: LJMD_STRESS needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_BATCH_STRESS_MAX_SNAPSHOTS) &
      stop 'md_simulation_many: more sampling instants than LJMD_BATCH_STRESS_MAX_SNAPSHOTS.'
    call ljmd_batch_check(ljmd_batch_stress_configure(batch, int(n_snapshots_expected, c_int32_t), 0_c_int32_t), batch, &
                          'ljmd_batch_stress_configure')
    allocate(stress_times(n_snapshots_expected, n_runs))
  end if
  if (heatflux_on) then
    if (n_snapshots_expected < 1) stop 'md_simulation_many: LJMD_HEATFLUX needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS) &
      stop 'md_simulation_many: more sampling instants than LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS.'
    call ljmd_batch_check(ljmd_batch_heatflux_configure(batch, int(n_snapshots_expected, c_int32_t), 0_c_int32_t), batch, &
                          'ljmd_batch_heatflux_configure')
    allocate(heatflux_times(n_snapshots_expected, n_runs))
  end if
  if (rhok_n2max > 0) then
    ! one mode list for all runs; one snapshot per sampling instant that writes an rva.dat record, taken by hand
    if (n_snapshots_expected < 1) stop 'md_simulation_many: LJMD_RHOK_N2MAX needs at least one sampling instant.'
    if (n_snapshots_expected > LJMD_BATCH_RHOK_MAX_SNAPSHOTS) &
      stop 'md_simulation_many: more sampling instants than LJMD_BATCH_RHOK_MAX_SNAPSHOTS.'
    rhok_status = ljmd_rhok_select_modes(int(rhok_n2max, c_int32_t), int(rhok_per_shell, c_int32_t), 0_c_int32_t, c_null_ptr, &
                                         rhok_n_modes)
    if (rhok_status == LJMD_OK .or. rhok_n_modes < 1) call ljmd_check(rhok_status, c_null_ptr, 'ljmd_rhok_select_modes')
    if (rhok_n_modes > LJMD_RHOK_MAX_MODES) stop 'md_simulation_many: more modes than LJMD_RHOK_MAX_MODES: lower LJMD_RHOK_N2MAX.'
    allocate(rhok_modes(3, rhok_n_modes))
    call ljmd_check(ljmd_rhok_select_modes(int(rhok_n2max, c_int32_t), int(rhok_per_shell, c_int32_t), rhok_n_modes, &
                                           c_loc(rhok_modes), rhok_n_modes), c_null_ptr, 'ljmd_rhok_select_modes')
    call ljmd_batch_check(ljmd_batch_rhok_configure(batch, rhok_n_modes, c_loc(rhok_modes), &
                                                    int(n_snapshots_expected, c_int32_t), 0_c_int32_t), batch, &
                          'ljmd_batch_rhok_configure')
    allocate(rhok_times(n_snapshots_expected, n_runs))
  end if
  do i = 1, n_runs
    open(newunit=iu_rva(i), file=trim(run_dir(i)) // '/rva.dat', form='unformatted', status='replace', &
         action='write', iostat=ios)
    if (ios /= 0) stop 'md_simulation_many: cannot open rva.dat of a run.'
    write(iu_rva(i)) rparams(i)%n, rparams(i)%box_length, rparams(i)%dt, output_interval, n_snapshots_expected
    open(newunit=iu_out(i), file=trim(run_dir(i)) // '/instantaneous_energies.dat', status='replace', &
         action='write', iostat=ios)
    if (ios /= 0) stop 'md_simulation_many: cannot open instantaneous_energies.dat of a run.'
    write(iu_out(i), '(a)') '# time   epot   ekin   etot   T   P'
    call stats_begin(stats(i), rparams(i)%n, rparams(i)%volume, n_snapshots_expected)
  end do

  num_samples = 0
  step = 0
  call system_clock(c0, crate)
  ! segments of output_interval steps, each sampled at its last step -- the sampling instants of :361
  do while (step + output_interval <= total_steps)
    call ljmd_batch_check(ljmd_batch_steps(batch, int(output_interval, c_int32_t), int(output_interval, c_int32_t), &
                                           c_loc(s_epot), c_loc(s_ekin), c_loc(s_depot), c_loc(s_ddepot)), batch, &
                          'ljmd_batch_steps')
    do i = 1, n_runs
      do k = 1, output_interval
        time_run(i) = time_run(i) + rparams(i)%dt   ! accumulated as at :356, with the run's own dt
      end do
    end do
    step = step + output_interval
    if (step <= warmup_steps) cycle
    num_samples = num_samples + 1
    if (rdf_bins > 0) call ljmd_batch_check(ljmd_batch_rdf_accumulate(batch), batch, 'ljmd_batch_rdf_accumulate')
    if (tcf_max_lag > 0) call ljmd_batch_check(ljmd_batch_tcf_accumulate(batch), batch, 'ljmd_batch_tcf_accumulate')
    if (vh_max_lag > 0) call ljmd_batch_check(ljmd_batch_vanhove_accumulate(batch), batch, 'ljmd_batch_vanhove_accumulate')
    if (stress_on) then
      call ljmd_batch_check(ljmd_batch_stress_accumulate(batch), batch, 'ljmd_batch_stress_accumulate')
      stress_times(num_samples, :) = time_run
    end if
    if (heatflux_on) then
      call ljmd_batch_check(ljmd_batch_heatflux_accumulate(batch), batch, 'ljmd_batch_heatflux_accumulate')
      heatflux_times(num_samples, :) = time_run
    end if
    if (rhok_n2max > 0) then
      call ljmd_batch_check(ljmd_batch_rhok_accumulate(batch), batch, 'ljmd_batch_rhok_accumulate')
      rhok_times(num_samples, :) = time_run
    end if
    call ljmd_batch_check(ljmd_batch_get_state(batch, c_loc(rx), c_loc(ry), c_loc(rz), c_loc(ux), c_loc(uy), &
                                               c_loc(uz), c_loc(vx), c_loc(vy), c_loc(vz), c_loc(ax), c_loc(ay), &
                                               c_loc(az)), batch, 'ljmd_batch_get_state')
    do i = 1, n_runs
      call stats_push(stats(i), s_epot(i), s_ekin(i), s_depot(i), s_ddepot(i), temp_inst, press_inst)
      etot = s_epot(i) + s_ekin(i)
      time = time_run(i)
      write(iu_out(i), '(1pe13.6,5(2x,1pe13.6))') time, s_epot(i), s_ekin(i), etot, temp_inst, press_inst
      o = off(i)
      ni = rparams(i)%n
      write(iu_rva(i)) rx(o + 1:o + ni), ry(o + 1:o + ni), rz(o + 1:o + ni)
      write(iu_rva(i)) ux(o + 1:o + ni), uy(o + 1:o + ni), uz(o + 1:o + ni)
      write(iu_rva(i)) vx(o + 1:o + ni), vy(o + 1:o + ni), vz(o + 1:o + ni)
      write(iu_rva(i)) ax(o + 1:o + ni), ay(o + 1:o + ni), az(o + 1:o + ni)
    end do
  end do
  rest = total_steps - step                         ! the steps after the last sampling instant: nothing is sampled
  if (rest > 0) call ljmd_batch_check(ljmd_batch_steps(batch, int(rest, c_int32_t), 1_c_int32_t, c_null_ptr, &
                                                       c_null_ptr, c_null_ptr, c_null_ptr), batch, 'ljmd_batch_steps')
  call system_clock(c1)
  if (rdf_bins > 0) then
    allocate(rdf_hist(rdf_bins, n_runs))
    call ljmd_batch_check(ljmd_batch_rdf_read(batch, c_loc(rdf_hist), rdf_snapshots), batch, 'ljmd_batch_rdf_read')
  end if
  if (tcf_max_lag > 0) then
    allocate(tcf_msd(0:tcf_max_lag, n_runs), tcf_vacf(0:tcf_max_lag, n_runs), tcf_counts(0:tcf_max_lag))
    call ljmd_batch_check(ljmd_batch_tcf_read(batch, c_loc(tcf_msd), c_loc(tcf_vacf), c_loc(tcf_counts), &
                                              tcf_snapshots), batch, 'ljmd_batch_tcf_read')
  end if
  if (stress_on) then
    allocate(stress_p(6, n_runs, max(num_samples, 1)))
    call ljmd_batch_check(ljmd_batch_stress_read(batch, c_loc(stress_p), stress_snapshots), batch, 'ljmd_batch_stress_read')
    if (stress_snapshots /= num_samples) stop 'md_simulation_many: the pressure tensor series and the samples disagree.'
  end if
  if (heatflux_on) then
    allocate(heatflux_j(3, n_runs, max(num_samples, 1)), heatflux_parts(3, 3, n_runs, max(num_samples, 1)))
    call ljmd_batch_check(ljmd_batch_heatflux_read(batch, c_loc(heatflux_j), c_loc(heatflux_parts), heatflux_snapshots), &
                          batch, 'ljmd_batch_heatflux_read')
    if (heatflux_snapshots /= num_samples) stop 'md_simulation_many: the heat flux series and the samples disagree.'
  end if
  if (vh_max_lag > 0) then
    allocate(vh_r2(0:vh_max_lag, n_runs), vh_r4(0:vh_max_lag, n_runs), vh_counts(0:vh_max_lag), &
             vh_hist(0:vh_bins, 0:vh_max_lag, n_runs))
    call ljmd_batch_check(ljmd_batch_vanhove_read(batch, c_loc(vh_hist), c_loc(vh_r2), c_loc(vh_r4), c_loc(vh_counts), &
                                                  vh_snapshots), batch, 'ljmd_batch_vanhove_read')
  end if
  if (rhok_n2max > 0) then
    allocate(rhok_rho(2, rhok_n_modes, n_runs, max(num_samples, 1)))
    call ljmd_batch_check(ljmd_batch_rhok_read(batch, c_loc(rhok_rho), rhok_snapshots), batch, 'ljmd_batch_rhok_read')
    if (rhok_snapshots /= num_samples) stop 'md_simulation_many: the density mode series and the samples disagree.'
  end if
  call ljmd_batch_destroy(batch)
  do i = 1, n_runs
    close(iu_out(i))
    close(iu_rva(i))
  end do

  if (num_samples <= 0) stop 'md_simulation: no samples were taken (check warmup_steps/output_interval).'
  open(newunit=iu, file=runs_list, status='replace', action='write', iostat=ios)
  if (ios /= 0) stop 'md_simulation_many: cannot open outputs/several_runs.txt for writing.'
  write(iu, '(a)') '# List of MD run output directories (one per line)'
  write(iu, '(a)') '# Generated by run_many_md.f90'
  do i = 1, n_runs
    call write_run_statistics(trim(run_dir(i)), rparams(i), total_steps, output_interval, warmup_steps, stats(i))
    write(iu, '(a)') trim(run_dir(i))
  end do
  close(iu)
  if (rdf_bins > 0) then
    do i = 1, n_runs
      call write_rdf(i)
    end do
  end if
  if (tcf_max_lag > 0) then
    do i = 1, n_runs
      call write_msd_vacf_file(trim(run_dir(i)) // '/msd_vacf_gpu.dat', tcf_max_lag, output_interval, rparams(i)%dt, &
                               tcf_counts, tcf_msd(:, i), tcf_vacf(:, i))
    end do
  end if
  if (stress_on) then
    do i = 1, n_runs
      call write_stress(i)
    end do
  end if
  if (heatflux_on) then
    do i = 1, n_runs
      call write_heat_flux(i)
    end do
  end if
  if (vh_max_lag > 0) then
    do i = 1, n_runs
      call write_van_hove_file(trim(run_dir(i)) // '/van_hove_gpu.dat', rparams(i)%n, vh_max_lag, vh_bins, vh_rmax(i), &
                               output_interval, rparams(i)%dt, vh_counts, vh_r2(:, i), vh_r4(:, i), vh_hist(:, :, i))
    end do
  end if
  if (rhok_n2max > 0) then
    do i = 1, n_runs
      call write_density_modes(i)
    end do
  end if
  if (any_own) then
    write(*, '(a,i0,a,i0,a,i0,a,f12.2,a)') 'md_simulation_many_gpu: particles=', total, ' runs=', n_runs_c, &
      ' steps=', total_steps, '  ', dble(n_runs) * dble(total_steps) * dble(crate) / dble(max(c1 - c0, 1_8)), &
      ' run-steps/s'
  else
    write(*, '(a,i0,a,i0,a,i0,a,f12.2,a)') 'md_simulation_many_gpu: N=', params%n, ' runs=', n_runs_c, ' steps=', &
      total_steps, '  ', dble(n_runs) * dble(total_steps) * dble(crate) / dble(max(c1 - c0, 1_8)), ' run-steps/s'
  end if

contains

  ! run i's own outputs/run_NNNN/input_simulation_parameters.txt, if any: k, dt, L, rc_over_L of the run; its block 1
  ! must repeat the shared total_steps, output_interval and warmup_steps
  subroutine read_run_parameters(irun)
    integer, intent(in) :: irun
    character(len=128) :: filename
    integer(kind=int_kind) :: ts, oi, ws
    real(kind=dp_kind) :: rcl, tte
    filename = trim(run_dir(irun)) // '/input_simulation_parameters.txt'
    inquire(file=trim(filename), exist=own_params(irun))
    if (.not. own_params(irun)) then
      rparams(irun) = params
      target_run(irun) = target_total_energy
      return
    end if
    call read_simulation_parameters(trim(filename), rparams(irun), ts, oi, ws, rcl, tte)
    target_run(irun) = tte
    if (ts /= total_steps .or. oi /= output_interval .or. ws /= warmup_steps) then
      write(*, '(a,a,a)') 'md_simulation_many_gpu: ', trim(filename), ': total_steps, output_interval and '// &
        'warmup_steps must equal those of inputs/input_simulation_parameters.txt (all runs step together)'
      stop 'md_simulation_many: a run''s steps block differs from the shared input.'
    end if
    if (rparams(irun)%n > LJMD_BATCH_MAX_N) then
      write(*, '(a,a,a,i0,a,i0,a)') 'md_simulation_many_gpu: ', trim(filename), ': N = ', rparams(irun)%n, &
        ' exceeds LJMD_BATCH_MAX_N (', LJMD_BATCH_MAX_N, ')'
      stop 'md_simulation_many: a run''s N is too large for a batch.'
    end if
    write(*, '(a,a,a,i0,a,1pe13.6,a,1pe13.6,a,1pe13.6)') 'md_simulation_many_gpu: ', trim(run_dir(irun)), &
      ' uses its own input_simulation_parameters.txt: N=', rparams(irun)%n, ' L=', rparams(irun)%box_length, &
      ' dt=', rparams(irun)%dt, ' rc=', rparams(irun)%rc
  end subroutine read_run_parameters

  ! run i's rdf_gpu.dat (md_run_outputs: write_rdf_file), up to half its box
  subroutine write_rdf(irun)
    integer, intent(in) :: irun
    call write_rdf_file(trim(run_dir(irun)) // '/rdf_gpu.dat', rparams(irun)%n, rparams(irun)%box_length, &
                        0.5d0 * rparams(irun)%box_length, rdf_bins, rdf_hist(:, irun), rdf_snapshots)
  end subroutine write_rdf

  ! run i's pressure_tensor_gpu.dat and, with LJMD_STRESS_MAX_LAG > 0, stress_acf_gpu.dat: what md_simulation_gpu writes
  ! for one run (md_run_outputs: write_pressure_tensor_file, write_stress_acf_file), from the run's rows of the series
  subroutine write_stress(irun)
    integer, intent(in) :: irun
    real(c_double), allocatable, target :: p(:, :), c(:, :), shear(:), normal(:)
    real(kind=dp_kind) :: mean_temp, std_temp
    integer :: ns, lags
    ns = int(num_samples)
    allocate(p(6, ns))
    p = stress_p(:, irun, 1:ns)
    call write_pressure_tensor_file(trim(run_dir(irun)) // '/pressure_tensor_gpu.dat', ns, stress_times(1:ns, irun), p)
    if (stress_max_lag <= 0 .or. ns < 2) return
    ! the three shear components, then the three normal differences, as the velocity of one particle: [1, snapshots] each
    allocate(c(ns, 6))
    c(:, 1) = p(4, :)
    c(:, 2) = p(5, :)
    c(:, 3) = p(6, :)
    c(:, 4) = 0.5d0 * (p(1, :) - p(2, :))
    c(:, 5) = 0.5d0 * (p(2, :) - p(3, :))
    c(:, 6) = 0.5d0 * (p(3, :) - p(1, :))
    lags = min(stress_max_lag, ns - 1)
    allocate(shear(0:lags), normal(0:lags))
    call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(ns, c_int32_t), 1_c_int32_t, c_loc(c(1, 1)), c_loc(c(1, 2)), &
                                             c_loc(c(1, 3)), int(lags, c_int32_t), 1_c_int32_t, c_loc(shear)), c_null_ptr, &
                    'ljmd_time_origin_average')
    call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(ns, c_int32_t), 1_c_int32_t, c_loc(c(1, 4)), c_loc(c(1, 5)), &
                                             c_loc(c(1, 6)), int(lags, c_int32_t), 1_c_int32_t, c_loc(normal)), c_null_ptr, &
                    'ljmd_time_origin_average')
    shear = shear / 3.d0
    normal = normal / 3.d0
    call stats_mean_std(stats(irun), Q_T, mean_temp, std_temp)
    call write_stress_acf_file(trim(run_dir(irun)) // '/stress_acf_gpu.dat', lags, output_interval, rparams(irun)%dt, &
                               rparams(irun)%volume, mean_temp, shear, normal)
  end subroutine write_stress

  ! run i's heat_flux_gpu.dat and, with LJMD_HEATFLUX_MAX_LAG > 0, heat_flux_acf_gpu.dat: what md_simulation_gpu writes for
  ! one run (md_run_outputs: write_heat_flux_file, write_heat_flux_acf_file), from the run's rows of the series
  subroutine write_heat_flux(irun)
    integer, intent(in) :: irun
    real(c_double), allocatable, target :: j(:, :), parts(:, :, :), c(:, :), acf(:)
    real(kind=dp_kind) :: mean_temp, std_temp
    integer :: ns, lags
    ns = int(num_samples)
    allocate(j(3, ns), parts(3, 3, ns))
    j = heatflux_j(:, irun, 1:ns)
    parts = heatflux_parts(:, :, irun, 1:ns)
    call write_heat_flux_file(trim(run_dir(irun)) // '/heat_flux_gpu.dat', ns, heatflux_times(1:ns, irun), j, parts)
    if (heatflux_max_lag <= 0 .or. ns < 2) return
    ! the three components as the velocity of one particle: [1, snapshots] each
    allocate(c(ns, 3))
    c(:, 1) = j(1, :)
    c(:, 2) = j(2, :)
    c(:, 3) = j(3, :)
    lags = min(heatflux_max_lag, ns - 1)
    allocate(acf(0:lags))
    call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(ns, c_int32_t), 1_c_int32_t, c_loc(c(1, 1)), c_loc(c(1, 2)), &
                                             c_loc(c(1, 3)), int(lags, c_int32_t), 1_c_int32_t, c_loc(acf)), c_null_ptr, &
                    'ljmd_time_origin_average')
    acf = acf / 3.d0
    call stats_mean_std(stats(irun), Q_T, mean_temp, std_temp)
    call write_heat_flux_acf_file(trim(run_dir(irun)) // '/heat_flux_acf_gpu.dat', lags, output_interval, rparams(irun)%dt, &
                                  rparams(irun)%volume, mean_temp, acf)
  end subroutine write_heat_flux

  ! run i's density_modes_gpu.dat, structure_factor_gpu.dat and, with LJMD_RHOK_MAX_LAG > 0, intermediate_scattering_gpu.dat:
  ! what md_simulation_gpu writes for one run (md_run_outputs), from the run's rows of the series
  subroutine write_density_modes(irun)
    integer, intent(in) :: irun
    real(c_double), allocatable, target :: rho(:, :, :), re(:, :), im(:, :), zero(:, :), f(:, :), row(:)
    integer, allocatable :: first(:)
    integer :: ns, nm, lags, shells, sh, cnt
    ns = int(num_samples)
    nm = int(rhok_n_modes)
    allocate(rho(2, nm, ns))
    rho = rhok_rho(:, :, irun, 1:ns)
    call write_density_modes_file(trim(run_dir(irun)) // '/density_modes_gpu.dat', nm, rhok_modes, ns, rhok_times(1:ns, irun), rho)
    call write_structure_factor_file(trim(run_dir(irun)) // '/structure_factor_gpu.dat', rparams(irun)%n, &
                                     rparams(irun)%box_length, nm, rhok_modes, ns, rho)
    if (rhok_max_lag <= 0 .or. ns < 2) return
    ! per shell its modes as the particles and (Re, Im, 0) as the velocity: [modes of the shell, snapshots] each
    allocate(first(nm + 1))
    call density_mode_shells(nm, rhok_modes, shells, first)
    lags = min(rhok_max_lag, ns - 1)
    allocate(f(0:lags, shells), row(0:lags))
    do sh = 1, shells
      cnt = first(sh + 1) - first(sh)
      allocate(re(cnt, ns), im(cnt, ns), zero(cnt, ns))
      re = rho(1, first(sh):first(sh + 1) - 1, 1:ns)
      im = rho(2, first(sh):first(sh + 1) - 1, 1:ns)
      zero = 0.d0
      call ljmd_check(ljmd_time_origin_average(1_c_int32_t, int(ns, c_int32_t), int(cnt, c_int32_t), c_loc(re), c_loc(im), &
                                               c_loc(zero), int(lags, c_int32_t), 1_c_int32_t, c_loc(row)), c_null_ptr, &
                      'ljmd_time_origin_average')
      f(:, sh) = row / dble(rparams(irun)%n)
      deallocate(re, im, zero)
    end do
    call write_intermediate_scattering_file(trim(run_dir(irun)) // '/intermediate_scattering_gpu.dat', shells, lags, &
                                            output_interval, rparams(irun)%dt, f)
  end subroutine write_density_modes

  ! LJMD_SEED_BASE: every run's initial configuration on the device (seed_base + i - 1, the run's target_total_energy,
  ! the shared warmup_steps), then each run's rv_init_gpu.dat: the two records of rv_init.dat
  subroutine prepare_on_device()
    integer :: irun, iu_rv, ierr
    integer(kind=8) :: o0
    integer(kind=int_kind) :: ni0
    allocate(seeds_c(n_runs))
    do irun = 1, n_runs
      seeds_c(irun) = int(seed_base + irun - 1, c_int32_t)
    end do
    call ljmd_batch_check(ljmd_batch_prepare(batch, c_loc(seeds_c), c_loc(target_run), int(warmup_steps, c_int32_t), &
                                             c_null_ptr, c_null_ptr), batch, 'ljmd_batch_prepare')
    call ljmd_batch_check(ljmd_batch_get_state(batch, c_loc(rx), c_loc(ry), c_loc(rz), c_null_ptr, c_null_ptr, &
                                               c_null_ptr, c_loc(vx), c_loc(vy), c_loc(vz), c_null_ptr, c_null_ptr, &
                                               c_null_ptr), batch, 'ljmd_batch_get_state')
    do irun = 1, n_runs
      open(newunit=iu_rv, file=trim(run_dir(irun)) // '/rv_init_gpu.dat', form='unformatted', status='replace', &
           action='write', iostat=ierr)
      if (ierr /= 0) stop 'md_simulation_many: cannot open rv_init_gpu.dat of a run.'
      o0 = off(irun)
      ni0 = rparams(irun)%n
      write(iu_rv) rx(o0 + 1:o0 + ni0), ry(o0 + 1:o0 + ni0), rz(o0 + 1:o0 + ni0)
      write(iu_rv) vx(o0 + 1:o0 + ni0), vy(o0 + 1:o0 + ni0), vz(o0 + 1:o0 + ni0)
      close(iu_rv)
      write(*, '(a,a,a,i0)') 'md_simulation_many_gpu: ', trim(run_dir(irun)), ' prepared on the device with seed ', &
        seeds_c(irun)
    end do
  end subroutine prepare_on_device

  ! run i's rv_init.dat: record 1 = rx ry rz, record 2 = vx vy vz (md_initial_config_program.f90:285-286)
  subroutine read_rv_init(irun)
    integer, intent(in) :: irun
    character(len=128) :: filename
    logical :: own
    integer :: iu_in, ierr
    integer(kind=8) :: o0
    integer(kind=int_kind) :: ni0
    filename = trim(run_dir(irun)) // '/rv_init.dat'
    inquire(file=trim(filename), exist=own)
    if (.not. own) then
      if (rparams(irun)%n /= n) then
        write(*, '(a,a,a)') 'md_simulation_many_gpu: ', trim(run_dir(irun)), &
          ' has its own N but no rv_init.dat of its own'
        stop 'read_rv_init(): a run with its own N needs its own rv_init.dat.'
      end if
      filename = 'outputs/rv_init.dat'
      write(*, '(a,a,a)') 'md_simulation_many_gpu: ', trim(run_dir(irun)), &
        ' starts from the shared outputs/rv_init.dat (identical to every other run that does)'
    end if
    open(newunit=iu_in, file=trim(filename), form='unformatted', status='old', action='read', iostat=ierr)
    if (ierr /= 0) stop 'read_rv_init(): cannot open rv_init file.'
    o0 = off(irun)
    ni0 = rparams(irun)%n
    read(iu_in) rx(o0 + 1:o0 + ni0), ry(o0 + 1:o0 + ni0), rz(o0 + 1:o0 + ni0)
    read(iu_in) vx(o0 + 1:o0 + ni0), vy(o0 + 1:o0 + ni0), vz(o0 + 1:o0 + ni0)
    close(iu_in)
  end subroutine read_rv_init

end program md_simulation_many_gpu
