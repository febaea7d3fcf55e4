!==============================================================================
! ljmd_c_api -- ISO_C_BINDING interfaces of libljmd.so (include/ljmd.h).
!
! This is the whole "FFI" a Fortran host needs: plain pointers, sizes and scalars by
! value.  The two stateless entry points replace the reference's module procedures
!   compute_lj_potential_energy   scripts/physics/lj_potential_energy.f90:46
!   verlet_step                   scripts/physics/verlet.f90:41
! and are what the drop-in modules lj_potential_energy.f90 / verlet.f90 of this
! directory forward to.  The handle-based entry points keep the state resident in
! HBM and are used by the thin driver md_simulation_gpu.f90.
!==============================================================================
module ljmd_c_api
  use, intrinsic :: iso_c_binding
  implicit none
  private

  public :: ljmd_compute_lj_potential_energy, ljmd_verlet_step, ljmd_stateless_reset
  public :: ljmd_set_tail_corrections, ljmd_stateless_set_tail_corrections
  public :: ljmd_create, ljmd_create_multi, ljmd_destroy, ljmd_set_state, ljmd_set_accel, ljmd_set_unwrapped
  public :: ljmd_get_state, ljmd_compute_forces, ljmd_verlet_steps, ljmd_kinetic_energy
  public :: ljmd_last_error, ljmd_device_count, ljmd_profile_enable, ljmd_profile_read
  public :: ljmd_enqueue_steps, ljmd_enqueue_steps_sampled, ljmd_collect_steps, ljmd_snapshot_begin, ljmd_snapshot_end
  public :: ljmd_check, ljmd_error_text
  ! batch engine: many independent replicas on one device, of one (n, L, dt, rc) or each with its own (ljmd.h,
  ! ljmd_batch_*)
  public :: ljmd_batch_create, ljmd_batch_create_per_replica, ljmd_batch_offsets, ljmd_batch_destroy, ljmd_batch_last_error, ljmd_batch_set_state, ljmd_batch_set_accel
  public :: ljmd_batch_set_unwrapped, ljmd_batch_get_state, ljmd_batch_compute_forces, ljmd_batch_kinetic_energy
  public :: ljmd_batch_steps, ljmd_batch_set_tail_corrections, ljmd_batch_set_precision, ljmd_batch_profile_read
  public :: ljmd_batch_rdf_configure, ljmd_batch_rdf_accumulate, ljmd_batch_rdf_read, ljmd_batch_rdf_reset
  public :: ljmd_rdf_configure, ljmd_rdf_accumulate, ljmd_rdf_read, ljmd_rdf_reset, ljmd_rdf_profile_read
  public :: ljmd_tcf_configure, ljmd_tcf_accumulate, ljmd_tcf_read, ljmd_tcf_read_exact, ljmd_tcf_reset, ljmd_tcf_profile_read
  public :: ljmd_vanhove_configure, ljmd_vanhove_accumulate, ljmd_vanhove_read, ljmd_vanhove_read_exact, ljmd_vanhove_reset
  public :: ljmd_vanhove_profile_read
  public :: ljmd_stress_configure, ljmd_stress_accumulate, ljmd_stress_read, ljmd_stress_read_exact, ljmd_stress_reset
  public :: ljmd_stress_profile_read, ljmd_stress_from_exact, ljmd_time_origin_average
  public :: ljmd_heatflux_configure, ljmd_heatflux_accumulate, ljmd_heatflux_read, ljmd_heatflux_read_exact
  public :: ljmd_heatflux_reset, ljmd_heatflux_profile_read, ljmd_heatflux_from_exact
  public :: ljmd_rhok_select_modes, ljmd_rhok_configure, ljmd_rhok_accumulate, ljmd_rhok_read, ljmd_rhok_read_exact
  public :: ljmd_rhok_reset, ljmd_rhok_profile_read
  public :: ljmd_current_configure, ljmd_current_accumulate, ljmd_current_read, ljmd_current_read_exact
  public :: ljmd_current_reset, ljmd_current_profile_read
  public :: ljmd_batch_tcf_configure, ljmd_batch_tcf_accumulate, ljmd_batch_tcf_read, ljmd_batch_tcf_read_exact
  public :: ljmd_batch_tcf_reset, ljmd_tcf_from_exact, ljmd_batch_prepare
  public :: ljmd_batch_stress_configure, ljmd_batch_stress_accumulate, ljmd_batch_stress_read, ljmd_batch_stress_read_exact
  public :: ljmd_batch_stress_reset
  public :: ljmd_batch_heatflux_configure, ljmd_batch_heatflux_accumulate, ljmd_batch_heatflux_read
  public :: ljmd_batch_heatflux_read_exact, ljmd_batch_heatflux_reset
  public :: ljmd_batch_vanhove_configure, ljmd_batch_vanhove_accumulate, ljmd_batch_vanhove_read
  public :: ljmd_batch_vanhove_read_exact, ljmd_batch_vanhove_reset
  public :: ljmd_batch_rhok_configure, ljmd_batch_rhok_accumulate, ljmd_batch_rhok_read, ljmd_batch_rhok_read_exact
  public :: ljmd_batch_rhok_reset, ljmd_batch_rhok_profile_read
  public :: ljmd_batch_check, ljmd_batch_error_text

  integer(c_int), parameter, public :: LJMD_OK = 0
  integer(c_int32_t), parameter, public :: LJMD_PRECISION_FP64 = 0
  integer(c_int32_t), parameter, public :: LJMD_PRECISION_FP64_REPRODUCIBLE = 2   ! exact fixed-point sums (ljmd.h)
  integer(c_int32_t), parameter, public :: LJMD_MAX_PENDING_STEPS = 4096
  integer(c_int32_t), parameter, public :: LJMD_BATCH_MAX_N = 4096
  integer(c_int32_t), parameter, public :: LJMD_TCF_MAX_LAG = 4096
  integer(c_int32_t), parameter, public :: LJMD_TCF_MAX_ORIGINS = 512
  integer(c_int32_t), parameter, public :: LJMD_VANHOVE_MAX_LAG = 4096
  integer(c_int32_t), parameter, public :: LJMD_VANHOVE_MAX_ORIGINS = 512
  integer(c_int32_t), parameter, public :: LJMD_VANHOVE_MAX_BINS = 4096
  integer(c_int32_t), parameter, public :: LJMD_BATCH_VANHOVE_MAX_LAG = 4096
  integer(c_int32_t), parameter, public :: LJMD_BATCH_VANHOVE_MAX_ORIGINS = 512
  integer(c_int32_t), parameter, public :: LJMD_BATCH_VANHOVE_MAX_BINS = 1024
  integer(c_int32_t), parameter, public :: LJMD_STRESS_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_BATCH_STRESS_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_HEATFLUX_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_RHOK_MAX_MODES = 4096
  integer(c_int32_t), parameter, public :: LJMD_RHOK_MAX_INDEX = 1023
  integer(c_int32_t), parameter, public :: LJMD_RHOK_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_RHOK_MAX_ENTRIES = 16777216
  integer(c_int32_t), parameter, public :: LJMD_CURRENT_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_CURRENT_MAX_ENTRIES = 4194304
  integer(c_int32_t), parameter, public :: LJMD_BATCH_RHOK_MAX_SNAPSHOTS = 262144
  integer(c_int32_t), parameter, public :: LJMD_BATCH_RHOK_MAX_ENTRIES = 16777216

  interface
    function ljmd_compute_lj_potential_energy(n, box_length, rc, rx, ry, rz, ax, ay, az, &
                                              epot, d_epot, dd_epot) bind(C, name="ljmd_compute_lj_potential_energy") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      integer(c_int32_t), value :: n
      real(c_double), value :: box_length, rc
      type(c_ptr), value :: rx, ry, rz, ax, ay, az
      real(c_double), intent(out) :: epot, d_epot, dd_epot
      integer(c_int) :: status
    end function

    function ljmd_verlet_step(n, box_length, dt, rc, rx, ry, rz, vx, vy, vz, ax, ay, az, &
                              epot, ekin, d_epot, dd_epot) bind(C, name="ljmd_verlet_step") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      integer(c_int32_t), value :: n
      real(c_double), value :: box_length, dt, rc
      type(c_ptr), value :: rx, ry, rz, vx, vy, vz, ax, ay, az
      real(c_double), intent(out) :: epot, ekin, d_epot, dd_epot
      integer(c_int) :: status
    end function

    subroutine ljmd_stateless_reset() bind(C, name="ljmd_stateless_reset")
    end subroutine

    ! the reference's use_tail_corrections (lj_potential_energy.f90:36): 0 = no tail constants in epot, d_epot, dd_epot
    subroutine ljmd_stateless_set_tail_corrections(on) bind(C, name="ljmd_stateless_set_tail_corrections")
      import :: c_int32_t
      integer(c_int32_t), value :: on
    end subroutine

    function ljmd_set_tail_corrections(handle, on) bind(C, name="ljmd_set_tail_corrections") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: on
      integer(c_int) :: status
    end function

    function ljmd_create(handle, n, box_length, dt, rc, precision_mode, device, rank, n_ranks) &
        bind(C, name="ljmd_create") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), intent(out) :: handle
      integer(c_int32_t), value :: n, precision_mode, device, rank, n_ranks
      real(c_double), value :: box_length, dt, rc
      integer(c_int) :: status
    end function

    ! one process, n_gpus devices (devices = c_null_ptr: 0 .. n_gpus-1); same entry points afterwards
    function ljmd_create_multi(handle, n, box_length, dt, rc, precision_mode, n_gpus, devices) &
        bind(C, name="ljmd_create_multi") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), intent(out) :: handle
      integer(c_int32_t), value :: n, precision_mode, n_gpus
      real(c_double), value :: box_length, dt, rc
      type(c_ptr), value :: devices
      integer(c_int) :: status
    end function

    subroutine ljmd_destroy(handle) bind(C, name="ljmd_destroy")
      import :: c_ptr
      type(c_ptr), value :: handle
    end subroutine

    function ljmd_set_state(handle, rx, ry, rz, vx, vy, vz) bind(C, name="ljmd_set_state") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, rx, ry, rz, vx, vy, vz
      integer(c_int) :: status
    end function

    function ljmd_set_accel(handle, ax, ay, az) bind(C, name="ljmd_set_accel") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, ax, ay, az
      integer(c_int) :: status
    end function

    function ljmd_set_unwrapped(handle, ux, uy, uz) bind(C, name="ljmd_set_unwrapped") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, ux, uy, uz
      integer(c_int) :: status
    end function

    function ljmd_get_state(handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az) &
        bind(C, name="ljmd_get_state") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az
      integer(c_int) :: status
    end function

    function ljmd_compute_forces(handle, epot, d_epot, dd_epot) bind(C, name="ljmd_compute_forces") result(status)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: epot, d_epot, dd_epot
      integer(c_int) :: status
    end function

    function ljmd_verlet_steps(handle, nsteps, epot, ekin, d_epot, dd_epot) &
        bind(C, name="ljmd_verlet_steps") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nsteps
      type(c_ptr), value :: epot, ekin, d_epot, dd_epot      ! each c_null_ptr or real(c_double)(nsteps)
      integer(c_int) :: status
    end function

    ! asynchronous production loop: enqueue returns at once, collect waits for the engine's stream
    function ljmd_enqueue_steps(handle, nsteps) bind(C, name="ljmd_enqueue_steps") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nsteps
      integer(c_int) :: status
    end function

    ! the same, the potential-energy sums evaluated on the LAST step only (the one the caller samples)
    function ljmd_enqueue_steps_sampled(handle, nsteps) bind(C, name="ljmd_enqueue_steps_sampled") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nsteps
      integer(c_int) :: status
    end function

    function ljmd_collect_steps(handle, nsteps, epot, ekin, d_epot, dd_epot) &
        bind(C, name="ljmd_collect_steps") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nsteps
      type(c_ptr), value :: epot, ekin, d_epot, dd_epot      ! each c_null_ptr or real(c_double)(nsteps)
      integer(c_int) :: status
    end function

    ! snapshot of r, ru, v, a: begin = stream-ordered freeze + transfer on a second stream (returns
    ! at once), end = wait for that transfer only and deliver the arrays
    function ljmd_snapshot_begin(handle) bind(C, name="ljmd_snapshot_begin") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_snapshot_end(handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az) &
        bind(C, name="ljmd_snapshot_end") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az
      integer(c_int) :: status
    end function

    function ljmd_kinetic_energy(handle, ekin) bind(C, name="ljmd_kinetic_energy") result(status)
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: ekin
      integer(c_int) :: status
    end function

    function ljmd_last_error(handle) bind(C, name="ljmd_last_error") result(msg)
      import :: c_ptr
      type(c_ptr), value :: handle
      type(c_ptr) :: msg
    end function

    function ljmd_device_count() bind(C, name="ljmd_device_count") result(n)
      import :: c_int32_t
      integer(c_int32_t) :: n
    end function

    function ljmd_profile_enable(handle, on) bind(C, name="ljmd_profile_enable") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: on
      integer(c_int) :: status
    end function

    function ljmd_profile_read(handle, ms_avg, launches) bind(C, name="ljmd_profile_read") result(status)
      import :: c_int, c_int32_t, c_ptr, c_double
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: ms_avg(4)
      integer(c_int32_t), intent(out) :: launches
      integer(c_int) :: status
    end function
    ! ---- batch engine: arrays of B*n doubles, replica-major; per-replica scalars [B]; ljmd_batch_steps' scalars
    ! [nsteps/sample_every][B] (Fortran: dimension(B, nsteps/sample_every)); c_null_ptr = not wanted
    function ljmd_batch_create(handle, n_replicas, n, box_length, dt, rc, precision_mode, device) &
        bind(C, name="ljmd_batch_create") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), intent(out) :: handle
      integer(c_int32_t), value :: n_replicas, n, precision_mode, device
      real(c_double), value :: box_length, dt, rc
      integer(c_int) :: status
    end function

    ! replica b with its own n(b), box_length(b), dt(b), rc(b); per-particle arrays hold the replicas one after another
    function ljmd_batch_create_per_replica(handle, n_replicas, n, box_length, dt, rc, precision_mode, device) &
        bind(C, name="ljmd_batch_create_per_replica") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), intent(out) :: handle
      integer(c_int32_t), value :: n_replicas, precision_mode, device
      integer(c_int32_t), intent(in) :: n(*)
      real(c_double), intent(in) :: box_length(*), dt(*), rc(*)
      integer(c_int) :: status
    end function

    ! offsets(b + 1) .. offsets(b + 2) - 1 (0-based elements): replica b's particles in every per-particle array
    function ljmd_batch_offsets(handle, offsets) bind(C, name="ljmd_batch_offsets") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: offsets(*)
      integer(c_int) :: status
    end function

    subroutine ljmd_batch_destroy(handle) bind(C, name="ljmd_batch_destroy")
      import :: c_ptr
      type(c_ptr), value :: handle
    end subroutine

    function ljmd_batch_last_error(handle) bind(C, name="ljmd_batch_last_error") result(text)
      import :: c_ptr
      type(c_ptr), value :: handle
      type(c_ptr) :: text
    end function

    function ljmd_batch_set_state(handle, rx, ry, rz, vx, vy, vz) bind(C, name="ljmd_batch_set_state") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, rx, ry, rz, vx, vy, vz
      integer(c_int) :: status
    end function

    function ljmd_batch_set_accel(handle, ax, ay, az) bind(C, name="ljmd_batch_set_accel") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, ax, ay, az
      integer(c_int) :: status
    end function

    function ljmd_batch_set_unwrapped(handle, ux, uy, uz) bind(C, name="ljmd_batch_set_unwrapped") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, ux, uy, uz
      integer(c_int) :: status
    end function

    function ljmd_batch_get_state(handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az) &
        bind(C, name="ljmd_batch_get_state") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az
      integer(c_int) :: status
    end function

    function ljmd_batch_compute_forces(handle, epot, d_epot, dd_epot) bind(C, name="ljmd_batch_compute_forces") &
        result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, epot, d_epot, dd_epot
      integer(c_int) :: status
    end function

    function ljmd_batch_kinetic_energy(handle, ekin) bind(C, name="ljmd_batch_kinetic_energy") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle, ekin
      integer(c_int) :: status
    end function

    function ljmd_batch_steps(handle, nsteps, sample_every, epot, ekin, d_epot, dd_epot) &
        bind(C, name="ljmd_batch_steps") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, epot, ekin, d_epot, dd_epot
      integer(c_int32_t), value :: nsteps, sample_every
      integer(c_int) :: status
    end function

    function ljmd_batch_set_tail_corrections(handle, on) bind(C, name="ljmd_batch_set_tail_corrections") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: on
      integer(c_int) :: status
    end function

    ! LJMD_PRECISION_FP64 or LJMD_PRECISION_FP64_REPRODUCIBLE; a change of mode asks for ljmd_batch_set_state again
    function ljmd_batch_set_precision(handle, precision_mode) bind(C, name="ljmd_batch_set_precision") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: precision_mode
      integer(c_int) :: status
    end function

    function ljmd_batch_profile_read(handle, kernel_ms, launches) bind(C, name="ljmd_batch_profile_read") &
        result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int32_t), intent(out) :: launches
      integer(c_int) :: status
    end function

    ! g(r) of the system resident on an engine handle (ljmd.h: ljmd_rdf_*): hist = c_loc of nbins 64-bit counts
    function ljmd_rdf_configure(handle, nbins, rmax) bind(C, name="ljmd_rdf_configure") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: nbins
      real(c_double), value :: rmax
      integer(c_int) :: status
    end function

    function ljmd_rdf_accumulate(handle) bind(C, name="ljmd_rdf_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_rdf_read(handle, hist, n_snapshots) bind(C, name="ljmd_rdf_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_rdf_reset(handle) bind(C, name="ljmd_rdf_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_rdf_profile_read(handle, tile_pairs_visited, tile_pairs_total, kernel_ms) &
        bind(C, name="ljmd_rdf_profile_read") result(status)
      import :: c_int, c_int64_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: tile_pairs_visited, tile_pairs_total
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! MSD / VACF of the system resident on a one-rank engine handle (ljmd.h: ljmd_tcf_*); msd, vacf, counts = c_loc of
    ! max_lag + 1 values, words [3, max_lag + 1, 2] in Fortran order; c_null_ptr skips an output
    function ljmd_tcf_configure(handle, max_lag, origin_stride) bind(C, name="ljmd_tcf_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_lag, origin_stride
      integer(c_int) :: status
    end function

    function ljmd_tcf_accumulate(handle) bind(C, name="ljmd_tcf_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_tcf_read(handle, msd, vacf, counts, n_snapshots) bind(C, name="ljmd_tcf_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, msd, vacf, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_tcf_read_exact(handle, words, counts, n_snapshots) bind(C, name="ljmd_tcf_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_tcf_reset(handle) bind(C, name="ljmd_tcf_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_tcf_profile_read(handle, kernel_ms, origins_live) bind(C, name="ljmd_tcf_profile_read") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int32_t), intent(out) :: origins_live
      integer(c_int) :: status
    end function

    ! van Hove self-correlation of the system resident on a one-rank engine handle (ljmd.h: ljmd_vanhove_*); hist = c_loc
    ! of [nbins + 1, max_lag + 1] 64-bit counts in Fortran order (the overflow column last), r2, r4, counts = c_loc of
    ! max_lag + 1 values, words [3, max_lag + 1, 2] in Fortran order; c_null_ptr skips an output
    function ljmd_vanhove_configure(handle, max_lag, origin_stride, nbins, rmax) bind(C, name="ljmd_vanhove_configure") &
        result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_lag, origin_stride, nbins
      real(c_double), value :: rmax
      integer(c_int) :: status
    end function

    function ljmd_vanhove_accumulate(handle) bind(C, name="ljmd_vanhove_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_vanhove_read(handle, hist, r2, r4, counts, n_snapshots) bind(C, name="ljmd_vanhove_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist, r2, r4, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_vanhove_read_exact(handle, hist, words, counts, n_snapshots) bind(C, name="ljmd_vanhove_read_exact") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist, words, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_vanhove_reset(handle) bind(C, name="ljmd_vanhove_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_vanhove_profile_read(handle, kernel_ms, origins_live) bind(C, name="ljmd_vanhove_profile_read") result(status)
      import :: c_int, c_int32_t, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int32_t), intent(out) :: origins_live
      integer(c_int) :: status
    end function

    ! pressure tensor of the system resident on an engine handle (ljmd.h: ljmd_stress_*); p = c_loc of [6, n_snapshots]
    ! doubles, words = c_loc of [3, 12, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_stress_configure(handle, max_snapshots) bind(C, name="ljmd_stress_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_snapshots
      integer(c_int) :: status
    end function

    function ljmd_stress_accumulate(handle) bind(C, name="ljmd_stress_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_stress_read(handle, p, n_snapshots) bind(C, name="ljmd_stress_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, p
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_stress_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_stress_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_stress_reset(handle) bind(C, name="ljmd_stress_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_stress_profile_read(handle, tile_pairs_visited, tile_pairs_total, kernel_ms) &
        bind(C, name="ljmd_stress_profile_read") result(status)
      import :: c_int, c_int64_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: tile_pairs_visited, tile_pairs_total
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! host only: words = c_loc of the [3, 12] words of one snapshot, out6 = c_loc of 6 doubles
    function ljmd_stress_from_exact(words, box_length, out6) bind(C, name="ljmd_stress_from_exact") result(status)
      import :: c_int, c_double, c_ptr
      type(c_ptr), value :: words, out6
      real(c_double), value :: box_length
      integer(c_int) :: status
    end function

    ! heat flux of the system resident on a one-rank engine handle (ljmd.h: ljmd_heatflux_*); j = c_loc of
    ! [3, n_snapshots] doubles, parts = c_loc of [3 axes, 3 parts, n_snapshots] doubles (convective, potential,
    ! collisional), words = c_loc of [3, 9, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_heatflux_configure(handle, max_snapshots) bind(C, name="ljmd_heatflux_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_snapshots
      integer(c_int) :: status
    end function

    function ljmd_heatflux_accumulate(handle) bind(C, name="ljmd_heatflux_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_heatflux_read(handle, j, parts, n_snapshots) bind(C, name="ljmd_heatflux_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, j, parts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_heatflux_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_heatflux_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_heatflux_reset(handle) bind(C, name="ljmd_heatflux_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_heatflux_profile_read(handle, tile_pairs_visited, tile_pairs_total, kernel_ms) &
        bind(C, name="ljmd_heatflux_profile_read") result(status)
      import :: c_int, c_int64_t, c_double, c_ptr
      type(c_ptr), value :: handle
      integer(c_int64_t), intent(out) :: tile_pairs_visited, tile_pairs_total
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! host only: one snapshot's words [3, 9] -> j[3] and, unless c_null_ptr, parts [3 axes, 3 parts]
    function ljmd_heatflux_from_exact(words, box_length, j3, parts9) bind(C, name="ljmd_heatflux_from_exact") result(status)
      import :: c_int, c_double, c_ptr
      type(c_ptr), value :: words, j3, parts9
      real(c_double), value :: box_length
      integer(c_int) :: status
    end function

    ! density modes of the system resident on a one-rank engine handle (ljmd.h: ljmd_rhok_*); modes = c_loc of
    ! [3, n_modes] 32-bit integers, rho = c_loc of [2, n_modes, n_snapshots] doubles (Re, Im), words = c_loc of
    ! [3, 2, n_modes, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_rhok_select_modes(n2_max, per_shell, capacity, modes, n_modes) bind(C, name="ljmd_rhok_select_modes") &
        result(status)
      import :: c_int, c_int32_t, c_ptr
      integer(c_int32_t), value :: n2_max, per_shell, capacity
      type(c_ptr), value :: modes
      integer(c_int32_t), intent(out) :: n_modes
      integer(c_int) :: status
    end function

    function ljmd_rhok_configure(handle, n_modes, modes, max_snapshots) bind(C, name="ljmd_rhok_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, modes
      integer(c_int32_t), value :: n_modes, max_snapshots
      integer(c_int) :: status
    end function

    function ljmd_rhok_accumulate(handle) bind(C, name="ljmd_rhok_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_rhok_read(handle, rho, n_snapshots) bind(C, name="ljmd_rhok_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, rho
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_rhok_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_rhok_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_rhok_reset(handle) bind(C, name="ljmd_rhok_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_rhok_profile_read(handle, kernel_ms) bind(C, name="ljmd_rhok_profile_read") result(status)
      import :: c_int, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! current modes of the system resident on a one-rank engine handle (ljmd.h: ljmd_current_*); modes = c_loc of
    ! [3, n_modes] 32-bit integers, j = c_loc of [2, 3, n_modes, n_snapshots] doubles ((Re, Im) of x, y, z), words = c_loc
    ! of [3, 2, 3, n_modes, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_current_configure(handle, n_modes, modes, max_snapshots) bind(C, name="ljmd_current_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, modes
      integer(c_int32_t), value :: n_modes, max_snapshots
      integer(c_int) :: status
    end function

    function ljmd_current_accumulate(handle) bind(C, name="ljmd_current_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_current_read(handle, j, n_snapshots) bind(C, name="ljmd_current_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, j
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_current_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_current_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_current_reset(handle) bind(C, name="ljmd_current_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_current_profile_read(handle, kernel_ms) bind(C, name="ljmd_current_profile_read") result(status)
      import :: c_int, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! time-origin averages of a host trajectory (ljmd.h): x, y, z = c_loc of [n, n_snap] doubles, out = c_loc of
    ! min(max_lag, n_snap - 1) + 1 doubles; kind 0 = MSD, 1 = VACF
    function ljmd_time_origin_average(kind, n_snap, n, x, y, z, max_lag, origin_stride, out) &
        bind(C, name="ljmd_time_origin_average") result(status)
      import :: c_int, c_int32_t, c_ptr
      integer(c_int32_t), value :: kind, n_snap, n, max_lag, origin_stride
      type(c_ptr), value :: x, y, z, out
      integer(c_int) :: status
    end function

    ! g(r) on the device: rmax = c_null_ptr (0.5 L of each replica) or B doubles; hist = [nbins, B] 64-bit counts
    function ljmd_batch_rdf_configure(handle, nbins, rmax, every) bind(C, name="ljmd_batch_rdf_configure") &
        result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, rmax
      integer(c_int32_t), value :: nbins, every
      integer(c_int) :: status
    end function

    function ljmd_batch_rdf_accumulate(handle) bind(C, name="ljmd_batch_rdf_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_rdf_read(handle, hist, n_snapshots) bind(C, name="ljmd_batch_rdf_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_rdf_reset(handle) bind(C, name="ljmd_batch_rdf_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    ! MSD / VACF on the device (ljmd.h: ljmd_batch_tcf_*); msd, vacf [max_lag + 1, B], counts [max_lag + 1],
    ! words [3, max_lag + 1, 2, B] in Fortran order; c_null_ptr skips an output
    ! initial configurations on the device: seeds(B) int32 and target_total_energy(B) required; epot0(B), ekin0(B) or
    ! c_null_ptr
    function ljmd_batch_prepare(handle, seeds, target_total_energy, warmup_steps, epot0, ekin0) &
        bind(C, name="ljmd_batch_prepare") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, seeds, target_total_energy, epot0, ekin0
      integer(c_int32_t), value :: warmup_steps
      integer(c_int) :: status
    end function

    function ljmd_batch_tcf_configure(handle, max_lag, origin_stride, every) bind(C, name="ljmd_batch_tcf_configure") &
        result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_lag, origin_stride, every
      integer(c_int) :: status
    end function

    function ljmd_batch_tcf_accumulate(handle) bind(C, name="ljmd_batch_tcf_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_tcf_read(handle, msd, vacf, counts, n_snapshots) bind(C, name="ljmd_batch_tcf_read") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, msd, vacf, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_tcf_read_exact(handle, words, counts, n_snapshots) bind(C, name="ljmd_batch_tcf_read_exact") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_tcf_reset(handle) bind(C, name="ljmd_batch_tcf_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    ! van Hove self-correlation of every replica of a batch handle (ljmd.h: ljmd_batch_vanhove_*); rmax = c_loc of B
    ! doubles; hist = c_loc of [nbins + 1, max_lag + 1, B] 64-bit counts in Fortran order (the overflow column last), r2,
    ! r4 [max_lag + 1, B], counts [max_lag + 1], words [3, max_lag + 1, 2, B]; c_null_ptr skips an output
    function ljmd_batch_vanhove_configure(handle, max_lag, origin_stride, nbins, rmax, every) &
        bind(C, name="ljmd_batch_vanhove_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_lag, origin_stride, nbins
      type(c_ptr), value :: rmax
      integer(c_int32_t), value :: every
      integer(c_int) :: status
    end function

    function ljmd_batch_vanhove_accumulate(handle) bind(C, name="ljmd_batch_vanhove_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_vanhove_read(handle, hist, r2, r4, counts, n_snapshots) bind(C, name="ljmd_batch_vanhove_read") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist, r2, r4, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_vanhove_read_exact(handle, hist, words, counts, n_snapshots) &
        bind(C, name="ljmd_batch_vanhove_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, hist, words, counts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_vanhove_reset(handle) bind(C, name="ljmd_batch_vanhove_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    ! density modes of every replica of a batch handle (ljmd.h: ljmd_batch_rhok_*); modes = c_loc of [3, n_modes] 32-bit
    ! integers, rho = c_loc of [2, n_modes, B, n_snapshots] doubles (Re, Im), words = c_loc of
    ! [3, 2, n_modes, B, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_batch_rhok_configure(handle, n_modes, modes, max_snapshots, every) &
        bind(C, name="ljmd_batch_rhok_configure") result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle, modes
      integer(c_int32_t), value :: n_modes, max_snapshots, every
      integer(c_int) :: status
    end function

    function ljmd_batch_rhok_accumulate(handle) bind(C, name="ljmd_batch_rhok_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_rhok_read(handle, rho, n_snapshots) bind(C, name="ljmd_batch_rhok_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, rho
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_rhok_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_batch_rhok_read_exact") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_rhok_reset(handle) bind(C, name="ljmd_batch_rhok_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_rhok_profile_read(handle, kernel_ms) bind(C, name="ljmd_batch_rhok_profile_read") result(status)
      import :: c_int, c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double), intent(out) :: kernel_ms
      integer(c_int) :: status
    end function

    ! pressure tensor of every replica of a batch handle (ljmd.h: ljmd_batch_stress_*); p = c_loc of [6, B, n_snapshots]
    ! doubles, words = c_loc of [3, 12, B, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_batch_stress_configure(handle, max_snapshots, every) bind(C, name="ljmd_batch_stress_configure") &
        result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_snapshots, every
      integer(c_int) :: status
    end function

    function ljmd_batch_stress_accumulate(handle) bind(C, name="ljmd_batch_stress_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_stress_read(handle, p, n_snapshots) bind(C, name="ljmd_batch_stress_read") result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, p
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_stress_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_batch_stress_read_exact") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_stress_reset(handle) bind(C, name="ljmd_batch_stress_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    ! heat flux of every replica of a batch handle (ljmd.h: ljmd_batch_heatflux_*); j = c_loc of [3, B, n_snapshots]
    ! doubles, parts = c_loc of [3, 3, B, n_snapshots] doubles (axis fastest, then convective / potential / collisional),
    ! words = c_loc of [3, 9, B, n_snapshots] 64-bit words in Fortran order; c_null_ptr skips an output
    function ljmd_batch_heatflux_configure(handle, max_snapshots, every) bind(C, name="ljmd_batch_heatflux_configure") &
        result(status)
      import :: c_int, c_int32_t, c_ptr
      type(c_ptr), value :: handle
      integer(c_int32_t), value :: max_snapshots, every
      integer(c_int) :: status
    end function

    function ljmd_batch_heatflux_accumulate(handle) bind(C, name="ljmd_batch_heatflux_accumulate") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_batch_heatflux_read(handle, j, parts, n_snapshots) bind(C, name="ljmd_batch_heatflux_read") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, j, parts
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_heatflux_read_exact(handle, words, n_snapshots) bind(C, name="ljmd_batch_heatflux_read_exact") &
        result(status)
      import :: c_int, c_int64_t, c_ptr
      type(c_ptr), value :: handle, words
      integer(c_int64_t), intent(out) :: n_snapshots
      integer(c_int) :: status
    end function

    function ljmd_batch_heatflux_reset(handle) bind(C, name="ljmd_batch_heatflux_reset") result(status)
      import :: c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: status
    end function

    function ljmd_tcf_from_exact(words, n, count, out) bind(C, name="ljmd_tcf_from_exact") result(status)
      import :: c_int, c_int32_t, c_int64_t, c_double
      integer(c_int64_t), intent(in) :: words(3)
      integer(c_int32_t), value :: n
      integer(c_int64_t), value :: count
      real(c_double), intent(out) :: out
      integer(c_int) :: status
    end function
  end interface

contains

  ! Text of the last error (handle = c_null_ptr: last error of a stateless call / failed create).
  function ljmd_error_text(handle) result(text)
    type(c_ptr), intent(in) :: handle
    character(len=:), allocatable :: text
    type(c_ptr) :: p
    character(kind=c_char), pointer :: chars(:)
    integer :: k, n
    p = ljmd_last_error(handle)
    text = ''
    if (.not. c_associated(p)) return
    call c_f_pointer(p, chars, [512])
    n = 0
    do k = 1, 512
      if (chars(k) == c_null_char) exit
      n = k
    end do
    allocate(character(len=n) :: text)
    do k = 1, n
      text(k:k) = chars(k)
    end do
  end function ljmd_error_text

  ! Text of the last error of a batch handle (handle = c_null_ptr: the last failed ljmd_batch_create of this thread).
  function ljmd_batch_error_text(handle) result(text)
    type(c_ptr), intent(in) :: handle
    character(len=:), allocatable :: text
    text = c_text(ljmd_batch_last_error(handle))
  end function ljmd_batch_error_text

  function c_text(p) result(text)
    type(c_ptr), intent(in) :: p
    character(len=:), allocatable :: text
    character(kind=c_char), pointer :: chars(:)
    integer :: k, n
    text = ''
    if (.not. c_associated(p)) return
    call c_f_pointer(p, chars, [512])
    n = 0
    do k = 1, 512
      if (chars(k) == c_null_char) exit
      n = k
    end do
    allocate(character(len=n) :: text)
    do k = 1, n
      text(k:k) = chars(k)
    end do
  end function c_text

  ! ljmd_check for a batch handle: the same `stop 'ljmd: ...'` convention
  subroutine ljmd_batch_check(status, handle, where)
    integer(c_int), intent(in) :: status
    type(c_ptr), intent(in) :: handle
    character(len=*), intent(in) :: where
    if (status /= LJMD_OK) then
      write(*, '(a)') 'ljmd: ' // where // ': ' // ljmd_batch_error_text(handle)
      stop 'ljmd: GPU hot path failed'
    end if
  end subroutine ljmd_batch_check

  ! The reference's error convention is `stop 'routine(): message'` (e.g.
  ! lj_potential_energy.f90:77-82): a non-zero status ends the program the same way.
  subroutine ljmd_check(status, handle, where)
    integer(c_int), intent(in) :: status
    type(c_ptr), intent(in) :: handle
    character(len=*), intent(in) :: where
    if (status /= LJMD_OK) then
      write(*, '(a)') 'ljmd: ' // where // ': ' // ljmd_error_text(handle)
      stop 'ljmd: GPU hot path failed'
    end if
  end subroutine ljmd_check

end module ljmd_c_api
