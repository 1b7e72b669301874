#include "LOD.h"

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdlib>

namespace slod
{
  // solver settings of the global steps (the reference: fine_solver_control / coarse CG, LOD.cc:990-998,1070-1075)
  constexpr double fem_rel_tol = 1e-12, lod_rel_tol = 1e-13;
  constexpr int    fem_max_iterations = 50000, lod_max_iterations = 5000;

  template <int dim, int spacedim>
  LOD<dim, spacedim>::LOD(const LODParameters<dim, spacedim> &par)
    : par(par)
  {
    if (const char *r = std::getenv("RANK"))
      this_mpi_process = (unsigned int)std::atoi(r);
    if (const char *w = std::getenv("WORLD_SIZE"))
      n_mpi_processes = (unsigned int)std::max(1, std::atoi(w));
  }

  template <int dim, int spacedim>
  LOD<dim, spacedim>::~LOD()
  {
    for (slod_lod_factor *f : factors)
      slod_lod_factor_destroy(f);
    slod_lod_receivers_destroy(receivers);
    slod_lod_receivers_destroy(ens_receivers);
    slod_lod_sources_destroy(sources);
    slod_lod_sources_destroy(ens_sources);
    for (void *p : device_arrays)
      (void)hipFree(p);
    slod_destroy(handle);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::check(const int status, const char *what) const
  {
    if (status < 0)
      throw std::runtime_error(std::string(what) + ": " + slod_last_error(handle));
  }

  template <int dim, int spacedim>
  template <typename T>
  T *LOD<dim, spacedim>::device_alloc(const std::size_t n)
  {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<std::size_t>(n, 1) * sizeof(T)) != hipSuccess)
      throw std::runtime_error("hipMalloc of a global vector failed");
    device_arrays.push_back(p);
    return static_cast<T *>(p);
  }

  // ---- receivers and the record of the time loops
  template <int dim, int spacedim>
  slod_lod_receivers *LOD<dim, spacedim>::make_receivers(const std::vector<ReceiverPoint> &points, const bool ensemble, const char *who)
  {
    if (ensemble ? !d_ens_basis : !d_basis)
      throw std::runtime_error(std::string(who) + (ensemble ? ": solve_ensemble comes first" :
                                                              ": compute_basis_function_candidates comes first"));
    const unsigned int    NE = (1u << par.n_global_refinements) * par.n_subdivisions, NEp = NE + 1;
    std::vector<uint32_t> begin(1, 0), node;
    std::vector<int32_t>  comp;
    std::vector<double>   weight;
    for (const ReceiverPoint &p : points)
      {
        if (!(p.x >= 0.0 && p.x <= 1.0 && p.y >= 0.0 && p.y <= 1.0))
          throw std::runtime_error(std::string(who) + ": a point outside the unit square");
        // the four bilinear terms of the element that holds the point; on the far boundary the missing node has weight 0
        const double       fx = p.x * NE, fy = p.y * NE;
        const unsigned int ex = std::min((unsigned int)fx, NE), ey = std::min((unsigned int)fy, NE);
        const unsigned int x1 = std::min(ex + 1, NE), y1 = std::min(ey + 1, NE);
        const double       tx = fx - ex, ty = fy - ey;
        const uint32_t     nd[4] = {ex + ey * NEp, x1 + ey * NEp, ex + y1 * NEp, x1 + y1 * NEp};
        const double       w[4] = {(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty};
        for (int k = 0; k < 4; ++k)
          {
            node.push_back(nd[k]);
            comp.push_back(p.component);
            weight.push_back(w[k]);
          }
        begin.push_back((uint32_t)node.size());
      }
    slod_lod_receivers *r = nullptr;
    if (ensemble)
      check(slod_lod_receivers_create(handle, (int)points.size(), begin.data(), node.data(), comp.data(), weight.data(), d_ens_basis,
                                      ens_stride, ens_member_stride, (int)par.n_members, &r),
            "slod_lod_receivers_create");
    else
      check(slod_lod_receivers_create(handle, (int)points.size(), begin.data(), node.data(), comp.data(), weight.data(), d_basis,
                                      basis_stride, 0, 1, &r),
            "slod_lod_receivers_create");
    return r;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::create_receivers(const std::vector<ReceiverPoint> &points, const bool ensemble)
  {
    slod_lod_receivers *&r = ensemble ? ens_receivers : receivers;
    slod_lod_receivers_destroy(r);
    r           = nullptr;
    r           = make_receivers(points, ensemble, "create_receivers");
    n_receivers = (unsigned int)points.size();
  }

  // ---- sources and the signal that drives the time loops
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::create_sources(const std::vector<ReceiverPoint> &points, const bool ensemble)
  {
    slod_lod_sources *&s = ensemble ? ens_sources : sources;
    slod_lod_sources_destroy(s);
    s                     = nullptr;
    slod_lod_receivers *r = make_receivers(points, ensemble, "create_sources");
    const int           rc = slod_lod_sources_create(handle, r, &s);
    slod_lod_receivers_destroy(r); // the sources own their copy of the rows
    check(rc, "slod_lod_sources_create");
    n_sources = (unsigned int)points.size();
  }

  template <int dim, int spacedim>
  bool LOD<dim, spacedim>::source_open(const unsigned int needed, const unsigned int columns, const bool ensemble)
  {
    drive_open = false;
    if (drive_samples == 0)
      return false;
    const unsigned int samples = drive_samples;
    drive_samples              = 0; // one-shot, as the library's
    if (ensemble ? !ens_sources : !sources)
      throw std::runtime_error("drive_next: create_sources comes first");
    if (samples < needed || drive_signal.size() < (std::size_t)samples * n_sources)
      throw std::runtime_error("drive_next: the signal is shorter than the samples of the loop");
    drive_ensemble = ensemble;
    drive_cols     = columns;
    std::vector<double> wide((std::size_t)needed * n_sources * columns);
    for (std::size_t i = 0; i < (std::size_t)needed * n_sources; ++i)
      for (unsigned int c = 0; c < columns; ++c)
        wide[i * columns + c] = drive_signal[i];
    if (wide.size() > d_signal_size) // kept for later loops; a longer one takes a new array
      {
        d_signal      = device_alloc<double>(wide.size());
        d_signal_size = wide.size();
      }
    if (hipMemcpy(d_signal, wide.data(), wide.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("drive_next: upload of the signal failed");
    drive_samples_open = needed;
    return drive_open = true;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::source_arm(const unsigned int first)
  {
    if (!drive_open)
      return;
    slod_lod_time_source src{};
    src.src           = drive_ensemble ? ens_sources : sources;
    src.ld_signal     = drive_cols;
    src.sample_stride = (std::size_t)n_sources * drive_cols;
    src.d_signal      = d_signal + (std::size_t)first * src.sample_stride;
    src.n_samples     = (int)(drive_samples_open - first);
    check(slod_lod_time_source_arm(handle, &src), "slod_lod_time_source_arm");
  }

  template <int dim, int spacedim>
  const double *LOD<dim, spacedim>::source_load(const double *d_load, double *d_out)
  {
    if (!drive_open)
      return d_load;
    if (drive_ensemble)
      check(slod_lod_inject_ensemble(handle, ens_sources, 0, (int)drive_cols, d_signal, drive_cols, d_load, drive_cols, d_out, drive_cols,
                                     nullptr),
            "slod_lod_inject_ensemble");
    else
      check(slod_lod_inject_multi(handle, sources, d_signal, drive_cols, (int)drive_cols, d_load, drive_cols, d_out, drive_cols, nullptr),
            "slod_lod_inject_multi");
    return d_out;
  }

  template <int dim, int spacedim>
  bool LOD<dim, spacedim>::record_open(const unsigned int n_steps, const unsigned int columns, const bool has_v, const bool ensemble)
  {
    trace_open = false;
    if (record_every == 0)
      return false;
    trace_every_ = record_every;
    record_every = 0; // one-shot, as the library's
    if (ensemble ? !ens_receivers : !receivers)
      throw std::runtime_error("record_next: create_receivers comes first");
    trace_ensemble  = ensemble;
    trace_nq        = has_v ? 2 : 1;
    trace_cols      = columns;
    trace_n_records = n_steps / trace_every_ + 1;
    const std::size_t n = (std::size_t)trace_n_records * trace_nq * n_receivers * trace_cols;
    if (n > d_trace_size) // kept for later records; a longer one takes a new array
      {
        d_trace      = device_alloc<double>(n);
        d_trace_size = n;
      }
    if (hipMemset(d_trace, 0, n * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("record_next: clearing the trace failed");
    host_trace.assign(n, 0.0);
    return trace_open = true;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::record_arm(const unsigned int n_steps)
  {
    if (!trace_open)
      return;
    slod_lod_time_record rec{};
    rec.recv          = trace_ensemble ? ens_receivers : receivers;
    rec.what          = trace_nq == 2 ? (SLOD_RECORD_U | SLOD_RECORD_V) : SLOD_RECORD_U;
    rec.every         = (int)trace_every_;
    rec.d_trace       = d_trace;
    rec.ld_trace      = trace_cols;
    rec.record_stride = (std::size_t)trace_nq * n_receivers * trace_cols;
    rec.capacity      = (int)(n_steps / trace_every_ + 1);
    check(slod_lod_time_record_arm(handle, &rec), "slod_lod_time_record_arm");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::record_state(const unsigned int steps_done, const double *d_u, const double *d_v)
  {
    if (!trace_open || steps_done % trace_every_ != 0)
      return;
    const std::size_t block = (std::size_t)n_receivers * trace_cols;
    double           *at = d_trace + (std::size_t)(steps_done / trace_every_) * trace_nq * block;
    const double     *x[2] = {d_u, d_v};
    for (unsigned int w = 0; w < trace_nq; ++w)
      if (trace_ensemble)
        check(slod_lod_observe_ensemble(handle, ens_receivers, 0, (int)trace_cols, x[w], trace_cols, at + w * block, trace_cols, nullptr),
              "slod_lod_observe_ensemble");
      else
        check(slod_lod_observe_multi(handle, receivers, x[w], trace_cols, (int)trace_cols, at + w * block, trace_cols, nullptr),
              "slod_lod_observe_multi");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::record_close()
  {
    if (!trace_open)
      return;
    trace_open = false;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(host_trace.data(), d_trace, host_trace.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("record_next: download of the trace failed");
  }

  // GridGenerator::hyper_cube + refine_global + evenly distributed partitioning (LOD.cc:110-119)
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::make_grid()
  {
    slod_config cfg{};
    cfg.dim                   = dim;
    cfg.spacedim              = spacedim;
    cfg.n_global_refinements  = (int32_t)par.n_global_refinements;
    cfg.n_subdivisions        = (int32_t)par.n_subdivisions;
    cfg.oversampling          = (int32_t)par.oversampling;
    cfg.lod_stabilization     = par.LOD_stabilization;
    cfg.constant_coefficients = par.constant_coefficients;
    cfg.projection_quirk      = par.projection_quirk;
    cfg.n_problems            = (int32_t)par.n_members;
    cfg.device                = par.device;
    slod_handle *h            = nullptr;
    if (slod_create(&cfg, &h) != SLOD_OK)
      throw std::runtime_error(std::string("slod_create: ") + slod_last_error(nullptr));
    handle = h;
    uint64_t b = 0, e = 0;
    check(slod_partition((uint64_t)slod_num_patches(handle), n_mpi_processes, this_mpi_process, &b, &e),
          "slod_partition");
    locally_owned_patches = {(unsigned int)b, (unsigned int)e};
  }

  // the FE spaces are fixed by (n_subdivisions, spacedim): nothing to build (LOD.cc:67-106)
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::make_fe()
  {}

  // LOD.cc:122-244
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::create_patches()
  {
    const unsigned int n_patches = (unsigned int)slod_num_patches(handle);
    patches.clear();
    patches.resize(n_patches);
    std::size_t size_biggest_patch = 0, size_tiniest_patch = n_patches;
    for (unsigned int id = 0; id < n_patches; ++id)
      {
        slod_patch_info info;
        check(slod_patch_layout(handle, id, &info), "slod_patch_layout");
        auto &patch = patches[id];
        patch.cells.resize((std::size_t)info.mx * info.my);
        check(slod_patch_cells(handle, id, patch.cells.data(), patch.cells.size()), "slod_patch_cells");
        size_biggest_patch = std::max(size_biggest_patch, patch.cells.size());
        size_tiniest_patch = std::min(size_tiniest_patch, patch.cells.size());
      }
    if (this_mpi_process == 0)
      std::cout << "Number of coarse cell = " << n_patches << ", number of patches = " << patches.size()
                << " (locally owned: " << locally_owned_patches.second - locally_owned_patches.first
                << ") \n"
                << "Patches size in (" << size_tiniest_patch << ", " << size_biggest_patch << ")"
                << std::endl; // LOD.cc:237-242
  }

  // LOD.cc:770-858
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::create_mesh_for_patch(Patch<dim> &current_patch)
  {
    const unsigned int id = (unsigned int)(&current_patch - patches.data());
    slod_patch_info    info;
    check(slod_patch_layout(handle, id, &info), "slod_patch_layout");
    PatchMesh &m = current_patch.sub_tria;
    m.x0         = info.x0;
    m.y0         = info.y0;
    m.mx         = info.mx;
    m.my         = info.my;
    m.nx         = info.nx;
    m.ny         = info.ny;
    for (int s = 0; s < 4; ++s)
      m.boundary_id[s] = info.side_domain[s] ? 0u : 99u;
    current_patch.dealii_to_lexicographic.resize(info.n_fine);
    check(slod_patch_dof_permutation(handle, id, current_patch.dealii_to_lexicographic.data(),
                                     current_patch.dealii_to_lexicographic.size()),
          "slod_patch_dof_permutation");
  }

  // LOD.cc:1380-1393
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::initialize_patches()
  {
    create_patches();
    for (unsigned int id = locally_owned_patches.first; id < locally_owned_patches.second; ++id)
      create_mesh_for_patch(patches[id]);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_stiffness(const unsigned int patch_id, std::vector<double> &stencil)
  {
    slod_patch_info info;
    check(slod_patch_layout(handle, patch_id, &info), "slod_patch_layout");
    stencil.assign((std::size_t)(info.n_fine / spacedim) * 9 * spacedim * spacedim, 0.0);
    check(slod_assemble_stiffness_for_patch(handle, patch_id, stencil.data()),
          "slod_assemble_stiffness_for_patch");
  }

  // the points of QIterated(QGauss<1>(2), n) on every fine element of the global grid, index (ey NE + ex) 4 + q
  template <int dim, int spacedim>
  std::vector<Point<dim>> LOD<dim, spacedim>::fine_quadrature_points() const
  {
    const unsigned int N  = 1u << par.n_global_refinements;
    const unsigned int NE = N * par.n_subdivisions;
    const double       hf = 1.0 / NE, g0 = 0.5 * (1.0 - 1.0 / std::sqrt(3.0)),
                 g1 = 0.5 * (1.0 + 1.0 / std::sqrt(3.0));
    std::vector<Point<dim>> points((std::size_t)NE * NE * 4);
    for (unsigned int ey = 0; ey < NE; ++ey)
      for (unsigned int ex = 0; ex < NE; ++ex)
        for (unsigned int q = 0; q < 4; ++q)
          {
            Point<dim> &p = points[((std::size_t)ey * NE + ex) * 4 + q];
            p(0)          = (ex + ((q & 1) ? g1 : g0)) * hf;
            p(1)          = (ey + ((q & 2) ? g1 : g0)) * hf;
          }
    return points;
  }

  // LOD.cc:296-768: the whole patch loop runs on the GPU
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::compute_basis_function_candidates()
  {
    // coefficient at the quadrature points of QIterated(QGauss<1>(2), n) on every fine
    // element of the global grid (what FEValues::get_quadrature_points feeds to
    // Alpha.value_list in Diffusion.h:154)
    const std::vector<Point<dim>> points = fine_quadrature_points();
    std::vector<double>           values;
    for (unsigned int field = 0; field < (unsigned int)spacedim; ++field)
      {
        coefficients_at_quadrature_points(field, points, values);
        check(slod_set_coefficient(handle, 0, (int)field, values.data(), 1, values.size(), 0),
              "slod_set_coefficient");
      }

    const auto                t0 = std::chrono::steady_clock::now();
    const unsigned int        n  = locally_owned_patches.second - locally_owned_patches.first;
    std::vector<uint32_t>     ids(n);
    std::vector<uint64_t>     offsets(n);
    std::vector<unsigned int> n_fine(n);
    uint64_t                  total = 0;
    for (unsigned int k = 0; k < n; ++k)
      {
        ids[k] = locally_owned_patches.first + k;
        slod_patch_info info;
        check(slod_patch_layout(handle, ids[k], &info), "slod_patch_layout");
        n_fine[k]  = (unsigned int)info.n_fine;
        offsets[k] = total;
        total += (uint64_t)spacedim * info.n_fine;
      }
    std::vector<double> basis(total), premult(total);
    check(slod_compute_basis(handle, ids.data(), n, basis.data(), premult.data(), offsets.data()),
          "slod_compute_basis");
    // scatter into Patch::basis_function(_premultiplied) in the patch-local deal.II numbering
    // (LOD.cc:592,754,764; consumer LOD.cc:931-962)
    for (unsigned int k = 0; k < n; ++k)
      {
        Patch<dim> &patch = patches[ids[k]];
        patch.basis_function.assign(spacedim, std::vector<double>(n_fine[k]));
        patch.basis_function_premultiplied.assign(spacedim, std::vector<double>(n_fine[k]));
        for (int d = 0; d < spacedim; ++d)
          for (unsigned int i = 0; i < n_fine[k]; ++i)
            {
              const unsigned int lex = patch.dealii_to_lexicographic[i];
              patch.basis_function[d][i] = basis[offsets[k] + (uint64_t)d * n_fine[k] + lex];
              patch.basis_function_premultiplied[d][i] = premult[offsets[k] + (uint64_t)d * n_fine[k] + lex];
            }
      }
    last_build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::run()
  {
    make_grid();
    make_fe();
    initialize_patches();
    create_random_problem_coefficients();
    compute_basis_function_candidates();
  }

  // LOD.cc:860-973.  Patch::basis_function(_premultiplied) back to the patch-lexicographic order of the
  // C-ABI, every patch at p * basis_stride of one device slab, then the block rows of A_LOD.
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_global_matrix()
  {
    const unsigned int n_patches = (unsigned int)patches.size();
    if (locally_owned_patches.first != 0 || locally_owned_patches.second != n_patches)
      throw std::runtime_error("assemble_global_matrix: the global steps need every patch in this process");
    // the uniform stride of the library's slabs (the full patch's vectors, also where the grid clips every patch): what
    // the plan of refresh_after_coefficient_change() writes to
    {
      slod_plan *empty = nullptr;
      check(slod_plan_create(handle, nullptr, 0, nullptr, &empty), "slod_plan_create");
      basis_stride = slod_plan_stride(empty);
      slod_plan_destroy(empty);
    }
    std::vector<double> basis(n_patches * basis_stride, 0.0), premult(basis.size(), 0.0);
    for (unsigned int p = 0; p < n_patches; ++p)
      {
        const Patch<dim> &patch  = patches[p];
        const std::size_t n_fine = patch.dealii_to_lexicographic.size();
        for (int d = 0; d < spacedim; ++d)
          for (std::size_t i = 0; i < n_fine; ++i)
            {
              const std::size_t at = p * basis_stride + d * n_fine + patch.dealii_to_lexicographic[i];
              basis[at]            = patch.basis_function[d][i];
              premult[at]          = patch.basis_function_premultiplied[d][i];
            }
      }
    d_basis   = device_alloc<double>(basis.size());
    d_premult = device_alloc<double>(premult.size());
    if (hipMemcpy(d_basis, basis.data(), basis.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_premult, premult.data(), premult.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("assemble_global_matrix: basis upload failed");
    const int cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    d_lod_values = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    d_lod_cols   = device_alloc<uint32_t>((std::size_t)n_patches * cap);
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    check(slod_lod_matrix(handle, rows.data(), n_patches, d_basis, d_premult, basis_stride, d_lod_values, d_lod_cols,
                          nullptr),
          "slod_lod_matrix");
  }

  // The coefficient changed in part of the domain: only the patches that see the change are rebuilt, and only the
  // entries of A_LOD (and M_LOD) with such a patch as row or column are recomputed, all in place on the device.
  template <int dim, int spacedim>
  unsigned int LOD<dim, spacedim>::refresh_after_coefficient_change()
  {
    if (!d_lod_values)
      throw std::runtime_error("refresh_after_coefficient_change: assemble_global_matrix comes first");
    const unsigned int n_patches = (unsigned int)patches.size();
    uint32_t          *d_dirty   = device_alloc<uint32_t>(n_patches);
    if (hipMemset(d_dirty, 0, n_patches * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("refresh_after_coefficient_change: clearing the dirty array failed");
    const std::vector<Point<dim>> points = fine_quadrature_points();
    std::vector<double>           values;
    for (unsigned int field = 0; field < (unsigned int)spacedim; ++field)
      {
        coefficients_at_quadrature_points(field, points, values);
        check(slod_update_coefficient(handle, 0, (int)field, values.data(), 1, values.size(), 0, d_dirty),
              "slod_update_coefficient");
      }
    slod_plan *plan = nullptr;
    const int  n_dirty = slod_plan_create_dirty(handle, 0, d_dirty, &plan);
    check(n_dirty, "slod_plan_create_dirty");
    int rc = slod_plan_execute(plan, d_basis, d_premult, nullptr);
    if (rc == SLOD_OK)
      rc = slod_plan_status(plan);
    slod_plan_destroy(plan);
    check(rc, "slod_plan_execute");
    check(slod_lod_matrix_update(handle, d_dirty, d_basis, d_premult, basis_stride, d_lod_values, 1, nullptr),
          "slod_lod_matrix_update");
    if (d_lod_mass)
      check(slod_lod_mass_matrix_update(handle, d_dirty, d_basis, basis_stride, nullptr, d_lod_mass, nullptr),
            "slod_lod_mass_matrix_update");
    // Patch::basis_function(_premultiplied) of the rebuilt patches, as compute_basis_function_candidates() leaves them
    std::vector<uint32_t> dirty((std::size_t)n_dirty);
    check(slod_dirty_patches(handle, d_dirty, dirty.data(), dirty.size()), "slod_dirty_patches"); // synchronises
    std::vector<double> basis, premult;
    for (const uint32_t p : dirty)
      {
        Patch<dim>       &patch  = patches[p];
        const std::size_t n_fine = patch.dealii_to_lexicographic.size();
        basis.resize(spacedim * n_fine);
        premult.resize(spacedim * n_fine);
        if (hipMemcpy(basis.data(), d_basis + p * basis_stride, basis.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(premult.data(), d_premult + p * basis_stride, premult.size() * sizeof(double), hipMemcpyDeviceToHost) !=
              hipSuccess)
          throw std::runtime_error("refresh_after_coefficient_change: basis download failed");
        for (int d = 0; d < spacedim; ++d)
          for (std::size_t i = 0; i < n_fine; ++i)
            {
              const std::size_t lex                    = d * n_fine + patch.dealii_to_lexicographic[i];
              patch.basis_function[d][i]               = basis[lex];
              patch.basis_function_premultiplied[d][i] = premult[lex];
            }
      }
    return (unsigned int)n_dirty;
  }

  template <int dim, int spacedim>
  std::vector<double> LOD<dim, spacedim>::lod_matrix_values() const
  {
    if (!d_lod_values)
      throw std::runtime_error("lod_matrix_values: assemble_global_matrix comes first");
    std::vector<double> v(patches.size() * (std::size_t)slod_lod_row_capacity(handle) * spacedim * spacedim);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(v.data(), d_lod_values, v.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("lod_matrix_values: download failed");
    return v;
  }

  template <int dim, int spacedim>
  std::vector<double> LOD<dim, spacedim>::lod_solution() const
  {
    if (!d_lod_u)
      throw std::runtime_error("lod_solution: solve comes first");
    std::vector<double> v(patches.size() * (std::size_t)spacedim);
    if (hipMemcpy(v.data(), d_lod_u, v.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("lod_solution: download failed");
    return v;
  }

  // LOD.cc:1004-1094 with the example's f = 1
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_and_solve_fem_problem()
  {
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    d_fem_rhs            = device_alloc<double>((NE + 1) * (NE + 1) * spacedim);
    d_fem_solution       = device_alloc<double>((NE + 1) * (NE + 1) * spacedim);
    check(slod_fem_rhs(handle, nullptr, d_fem_rhs, nullptr), "slod_fem_rhs");
    check(slod_fem_solve(handle, 0, d_fem_rhs, d_fem_solution, fem_rel_tol, fem_max_iterations, nullptr),
          "slod_fem_solve");
  }

  // LOD.cc:976-1002
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve()
  {
    if (!d_lod_values || !d_fem_rhs)
      throw std::runtime_error("solve: assemble_global_matrix and assemble_and_solve_fem_problem come first");
    const unsigned int    n_patches = (unsigned int)patches.size();
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    double *d_rhs = device_alloc<double>((std::size_t)n_patches * spacedim);
    d_lod_u       = device_alloc<double>((std::size_t)n_patches * spacedim);
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_rhs, nullptr), "slod_lod_rhs");
    check(slod_lod_solve(handle, d_lod_values, d_lod_cols, d_rhs, d_lod_u, lod_rel_tol, lod_max_iterations, nullptr),
          "slod_lod_solve");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::factor_for_reuse()
  {
    if (!d_lod_values)
      throw std::runtime_error("factor_for_reuse: assemble_global_matrix comes first");
    const std::size_t n_words = patches.size() * (std::size_t)slod_lod_row_capacity(handle) * spacedim * spacedim;
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>(n_words);
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    reuse_factor = factor_lod_matrix(d_lod_sym, false); // synchronises; this object destroys it
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_precond()
  {
    if (!reuse_factor || !d_fem_rhs)
      throw std::runtime_error("solve_precond: factor_for_reuse and assemble_and_solve_fem_problem come first");
    const unsigned int    n_patches = (unsigned int)patches.size();
    const std::size_t     n_coarse = (std::size_t)n_patches * spacedim;
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    if (!d_pcg_u) // u, the load and the Jacobi-CG solution, kept for the next call
      d_pcg_u = device_alloc<double>(3 * n_coarse);
    double *d_rhs = d_pcg_u + n_coarse, *d_jacobi_u = d_pcg_u + 2 * n_coarse;
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_rhs, nullptr), "slod_lod_rhs");
    check(slod_lod_solve_multi_precond(handle, reuse_factor, d_lod_sym, d_lod_cols, d_rhs, 1, 1, d_pcg_u, 1, lod_rel_tol,
                                       lod_max_iterations, &lod_pcg_iterations, nullptr),
          "slod_lod_solve_multi_precond");
    check(slod_lod_solve_multi(handle, d_lod_sym, d_lod_cols, d_rhs, 1, 1, d_jacobi_u, 1, lod_rel_tol, lod_max_iterations,
                               &lod_pcg_jacobi_iterations, nullptr),
          "slod_lod_solve_multi");
  }

  template <int dim, int spacedim>
  std::vector<double> LOD<dim, spacedim>::precond_solution() const
  {
    if (!d_pcg_u)
      throw std::runtime_error("precond_solution: solve_precond comes first");
    std::vector<double> v(patches.size() * (std::size_t)spacedim);
    if (hipMemcpy(v.data(), d_pcg_u, v.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("precond_solution: download failed");
    return v;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_ensemble_precond(const unsigned int member)
  {
    const int K = (int)par.n_members;
    if (!d_ens_values)
      throw std::runtime_error("solve_ensemble_precond: solve_ensemble comes first");
    if (member >= (unsigned int)K)
      throw std::runtime_error("solve_ensemble_precond: no such member");
    const std::size_t n_words = patches.size() * (std::size_t)slod_lod_row_capacity(handle) * spacedim * spacedim;
    const std::size_t n_coarse = patches.size() * (std::size_t)spacedim, ld = (std::size_t)K;
    if (!d_ens_sym)
      d_ens_sym = device_alloc<double>(n_words * K);
    if (!d_ens_pcg_u)
      d_ens_pcg_u = device_alloc<double>(n_coarse * K);
    double *d_u = d_ens_pcg_u;
    check(slod_lod_matrix_symmetrize_ensemble(handle, d_ens_values, ld, d_ens_cols, K, d_ens_sym, ld, nullptr),
          "slod_lod_matrix_symmetrize_ensemble");
    // the factor of one member: the ensemble of the one member `member` inside the wider array; freed before returning
    // (last_factor_info() keeps describing the factor of the caller's last direct loop)
    slod_lod_factor *f = nullptr;
    check(slod_lod_factor_create_ensemble(handle, d_ens_sym + member, ld, 1, d_ens_cols, nullptr, &f), "slod_lod_factor_create_ensemble");
    factors.push_back(f); // so that a throw below does not leak it
    lod_ens_pcg_iterations.assign(K, 0);
    lod_ens_pcg_jacobi.assign(K, 0);
    check(slod_lod_solve_ensemble_precond(handle, f, d_ens_sym, ld, d_ens_cols, d_ens_rhs, ld, K, d_u, ld, lod_rel_tol, lod_max_iterations,
                                          lod_ens_pcg_iterations.data(), nullptr),
          "slod_lod_solve_ensemble_precond");
    check(slod_lod_solve_ensemble(handle, d_ens_sym, ld, d_ens_cols, d_ens_rhs, ld, K, d_u, ld, lod_rel_tol, lod_max_iterations,
                                  lod_ens_pcg_jacobi.data(), nullptr),
          "slod_lod_solve_ensemble");
    factors.pop_back();
    slod_lod_factor_destroy(f);
  }

  // LOD.cc:1240-1260: u_LOD = C u_H, then error_LOD_FEMh.difference(u_h, u_LOD) in L2, H1, Linfty and energy
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::compare_lod_with_fem()
  {
    if (!d_lod_u || !d_fem_solution)
      throw std::runtime_error("compare_lod_with_fem: solve and assemble_and_solve_fem_problem come first");
    const std::size_t NE         = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    double           *d_lod_fine = device_alloc<double>((NE + 1) * (NE + 1) * spacedim);
    check(slod_lod_reconstruct(handle, d_basis, basis_stride, d_lod_u, d_lod_fine, nullptr), "slod_lod_reconstruct");
    check(slod_compute_error_norms(handle, 0, d_fem_solution, d_lod_fine, nullptr, nullptr, &lod_fem_error, nullptr),
          "slod_compute_error_norms");
    check(slod_compute_error_norms(handle, 0, d_fem_solution, nullptr, nullptr, nullptr, &fem_norms, nullptr),
          "slod_compute_error_norms");
  }

  // solve() for K loads: f_k at the points of quadrature_fine, [spacedim][NE][NE][4] per load
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_multi(const std::vector<const Function<dim> *> &loads)
  {
    if (!d_lod_values)
      throw std::runtime_error("solve_multi: assemble_global_matrix comes first");
    if (loads.empty())
      throw std::runtime_error("solve_multi: no load");
    const int          K = (int)loads.size();
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  n_qp = NE * NE * 4, fine_size = (NE + 1) * (NE + 1) * spacedim;
    const double       hf = 1.0 / NE, g0 = 0.5 * (1.0 - 1.0 / std::sqrt(3.0)), g1 = 0.5 * (1.0 + 1.0 / std::sqrt(3.0));
    std::vector<double> f_qp((std::size_t)K * spacedim * n_qp);
    for (int k = 0; k < K; ++k)
      for (int c = 0; c < spacedim; ++c)
        for (std::size_t ey = 0; ey < NE; ++ey)
          for (std::size_t ex = 0; ex < NE; ++ex)
            for (unsigned int q = 0; q < 4; ++q)
              {
                Point<dim> p;
                p(0) = (ex + ((q & 1) ? g1 : g0)) * hf;
                p(1) = (ey + ((q & 2) ? g1 : g0)) * hf;
                f_qp[((std::size_t)k * spacedim + c) * n_qp + (ey * NE + ex) * 4 + q] = loads[k]->value(p, (unsigned int)c);
              }
    double *d_f_qp = device_alloc<double>(f_qp.size());
    if (hipMemcpy(d_f_qp, f_qp.data(), f_qp.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("solve_multi: load upload failed");
    d_multi_fem_rhs = device_alloc<double>((std::size_t)K * fine_size);
    d_multi_fine    = device_alloc<double>((std::size_t)K * fine_size);
    for (int k = 0; k < K; ++k)
      check(slod_fem_rhs(handle, d_f_qp + (std::size_t)k * spacedim * n_qp, d_multi_fem_rhs + (std::size_t)k * fine_size, nullptr),
            "slod_fem_rhs");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    const std::size_t n_coarse = (std::size_t)n_patches * spacedim;
    double           *d_rhs = device_alloc<double>(n_coarse * K), *d_u = device_alloc<double>(n_coarse * K);
    check(slod_lod_rhs_multi(handle, rows.data(), n_patches, d_basis, basis_stride, d_multi_fem_rhs, fine_size, K, d_rhs,
                             (std::size_t)K, nullptr),
          "slod_lod_rhs_multi");
    lod_multi_iterations.assign(K, 0);
    lod_multi_residuals.assign(K, 0.0);
    check(slod_lod_solve_multi(handle, d_lod_values, d_lod_cols, d_rhs, (std::size_t)K, K, d_u, (std::size_t)K, lod_rel_tol,
                               lod_max_iterations, lod_multi_iterations.data(), lod_multi_residuals.data()),
          "slod_lod_solve_multi");
    check(slod_lod_reconstruct_multi(handle, d_basis, basis_stride, d_u, (std::size_t)K, K, d_multi_fine, fine_size, nullptr),
          "slod_lod_reconstruct_multi");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::compare_multi_with_fem()
  {
    if (!d_multi_fine)
      throw std::runtime_error("compare_multi_with_fem: solve_multi comes first");
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t fine_size = (NE + 1) * (NE + 1) * spacedim;
    double           *d_fem_u = device_alloc<double>(fine_size);
    lod_multi_fem_error.assign(lod_multi_iterations.size(), slod_error_norms{});
    for (std::size_t k = 0; k < lod_multi_fem_error.size(); ++k)
      {
        check(slod_fem_solve(handle, 0, d_multi_fem_rhs + k * fine_size, d_fem_u, fem_rel_tol, fem_max_iterations, nullptr),
              "slod_fem_solve");
        check(slod_compute_error_norms(handle, 0, d_fem_u, d_multi_fine + k * fine_size, nullptr, nullptr,
                                       &lod_multi_fem_error[k], nullptr),
              "slod_compute_error_norms");
      }
  }

  // plan -> matrix -> load -> solve -> reconstruct -> moments for all members, everything on the device
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_ensemble()
  {
    const int          K = (int)par.n_members;
    const unsigned int n_patches = (unsigned int)patches.size();
    if (!handle || locally_owned_patches.first != 0 || locally_owned_patches.second != n_patches)
      throw std::runtime_error("solve_ensemble: run() comes first, with every patch in this process");
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    // member 0 holds the coefficient of run(); the others are drawn now, at the same quadrature points
    const std::vector<Point<dim>> points = fine_quadrature_points();
    std::vector<double>           values;
    for (int k = 1; k < K; ++k)
      for (unsigned int field = 0; field < (unsigned int)spacedim; ++field)
        {
          member_coefficients_at_quadrature_points((unsigned int)k, field, points, values);
          check(slod_set_coefficient(handle, (uint32_t)k, (int)field, values.data(), 1, values.size(), 0), "slod_set_coefficient");
        }
    // one plan over gid = member * n_patches + patch: the ensemble slab, member k at k * n_patches * stride
    std::vector<uint32_t> gids((std::size_t)K * n_patches);
    for (std::size_t i = 0; i < gids.size(); ++i)
      gids[i] = (uint32_t)i;
    slod_plan *plan = nullptr;
    check(slod_plan_create(handle, gids.data(), gids.size(), nullptr, &plan), "slod_plan_create");
    const std::size_t stride = slod_plan_stride(plan), member_stride = n_patches * stride;
    double           *d_b = device_alloc<double>(K * member_stride), *d_q = device_alloc<double>(K * member_stride);
    int               rc = slod_plan_execute(plan, d_b, d_q, nullptr);
    if (rc == SLOD_OK)
      rc = slod_plan_status(plan);
    slod_plan_destroy(plan);
    check(rc, "slod_plan_execute");
    const int cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    double   *d_values = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim * K);
    uint32_t *d_cols   = device_alloc<uint32_t>((std::size_t)n_patches * cap);
    double   *d_load = device_alloc<double>(fine_size), *d_rhs = device_alloc<double>(n_coarse * K);
    double   *d_u = device_alloc<double>(n_coarse * K), *d_fine = device_alloc<double>(fine_size * K);
    double   *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    check(slod_lod_matrix_ensemble(handle, d_b, d_q, stride, member_stride, K, d_values, (std::size_t)K, d_cols, nullptr),
          "slod_lod_matrix_ensemble");
    check(slod_fem_rhs(handle, nullptr, d_load, nullptr), "slod_fem_rhs");
    check(slod_lod_rhs_ensemble(handle, d_b, stride, member_stride, K, d_load, 0, d_rhs, (std::size_t)K, nullptr),
          "slod_lod_rhs_ensemble");
    lod_ens_iterations.assign(K, 0);
    lod_ens_residuals.assign(K, 0.0);
    check(slod_lod_solve_ensemble(handle, d_values, (std::size_t)K, d_cols, d_rhs, (std::size_t)K, K, d_u, (std::size_t)K,
                                  lod_rel_tol, lod_max_iterations, lod_ens_iterations.data(), lod_ens_residuals.data()),
          "slod_lod_solve_ensemble");
    check(slod_lod_reconstruct_ensemble(handle, d_b, stride, member_stride, K, d_u, (std::size_t)K, d_fine, fine_size, nullptr),
          "slod_lod_reconstruct_ensemble");
    ensemble_moment_norms(d_fine, d_mean, d_var, ens_mean_norms, ens_dev_norms);
    ens_stride = stride, ens_member_stride = member_stride;
    d_ens_basis = d_b, d_ens_values = d_values, d_ens_cols = d_cols, d_ens_rhs = d_rhs;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::ensemble_moment_norms(const double *d_fine, double *d_mean, double *d_var, slod_error_norms &mean,
                                                 slod_error_norms &dev_norms)
  {
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t fine_size = (NE + 1) * (NE + 1) * spacedim;
    check(slod_ensemble_moments(handle, d_fine, fine_size, (int)par.n_members, fine_size, d_mean, d_var, nullptr),
          "slod_ensemble_moments");
    check(slod_compute_error_norms(handle, 0, d_mean, nullptr, nullptr, nullptr, &mean, nullptr),
          "slod_compute_error_norms"); // synchronises the handle's stream
    std::vector<double> dev(fine_size);
    if (hipMemcpy(dev.data(), d_var, fine_size * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("ensemble_moment_norms: variance download failed");
    for (double &v : dev)
      v = std::sqrt(v);
    if (hipMemcpy(d_var, dev.data(), fine_size * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("ensemble_moment_norms: deviation upload failed");
    check(slod_compute_error_norms(handle, 0, d_var, nullptr, nullptr, nullptr, &dev_norms, nullptr), "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_mass_matrix_ensemble()
  {
    if (!d_ens_values)
      throw std::runtime_error("assemble_mass_matrix_ensemble: solve_ensemble comes first");
    const int          K = (int)par.n_members;
    const unsigned int n_patches = (unsigned int)patches.size();
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_slots = (std::size_t)n_patches * cap;
    if (!d_ens_mass)
      d_ens_mass = device_alloc<double>(n_slots * spacedim * spacedim * K);
    // the call writes its columns; they must be those of the stiffness ensemble, which the loop uses for both matrices
    uint32_t *d_m_cols = nullptr;
    if (hipMalloc((void **)&d_m_cols, n_slots * sizeof(uint32_t)) != hipSuccess)
      throw std::runtime_error("assemble_mass_matrix_ensemble: hipMalloc of the columns failed");
    const int rc = slod_lod_mass_matrix_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, nullptr, 0, d_ens_mass,
                                                 (std::size_t)K, d_m_cols, nullptr);
    std::vector<uint32_t> m_cols(n_slots), a_cols(n_slots);
    const bool            copied = rc == SLOD_OK &&
                        hipMemcpy(m_cols.data(), d_m_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                        hipMemcpy(a_cols.data(), d_ens_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_m_cols);
    check(rc, "slod_lod_mass_matrix_ensemble");
    if (!copied || m_cols != a_cols)
      throw std::runtime_error("assemble_mass_matrix_ensemble: the pattern of M_LOD differs from that of A_LOD");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::ensemble_elliptic_solutions(double *d_ell_fine)
  {
    const int          K = (int)par.n_members;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_words = (std::size_t)n_patches * cap * spacedim * spacedim;
    double           *d_ell = device_alloc<double>(n_coarse * K);
    double *d_one = device_alloc<double>(n_words + 2 * n_coarse); // one member's matrix, load and elliptic solution
    // the elliptic solution of member k as solve() finds it: slod_lod_solve on the de-interleaved matrix and load
    // (the copies go through the host: this is the driver's reference, not the loop)
    std::vector<double> all_values(n_words * K), all_rhs(n_coarse * K), all_ell(n_coarse * K), one(n_words + n_coarse), u1(n_coarse);
    double             *d_rhs1 = d_one + n_words, *d_u1 = d_rhs1 + n_coarse;
    if (hipMemcpy(all_values.data(), d_ens_values, all_values.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(all_rhs.data(), d_ens_rhs, all_rhs.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("ensemble_elliptic_solutions: downloading the ensemble matrix failed");
    for (int k = 0; k < K; ++k)
      {
        for (std::size_t i = 0; i < n_words; ++i)
          one[i] = all_values[i * K + k];
        for (std::size_t i = 0; i < n_coarse; ++i)
          one[n_words + i] = all_rhs[i * K + k];
        if (hipMemcpy(d_one, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
          throw std::runtime_error("ensemble_elliptic_solutions: uploading a member failed");
        check(slod_lod_solve(handle, d_one, d_ens_cols, d_rhs1, d_u1, lod_rel_tol, lod_max_iterations, nullptr), "slod_lod_solve");
        if (hipMemcpy(u1.data(), d_u1, n_coarse * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          throw std::runtime_error("ensemble_elliptic_solutions: downloading a solution failed");
        for (std::size_t i = 0; i < n_coarse; ++i)
          all_ell[i * K + k] = u1[i];
      }
    if (hipMemcpy(d_ell, all_ell.data(), all_ell.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("ensemble_elliptic_solutions: uploading the elliptic solutions failed");
    check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, d_ell, (std::size_t)K, d_ell_fine,
                                        fine_size, nullptr),
          "slod_lod_reconstruct_ensemble");
    ens_lod_norms.assign(K, slod_error_norms{});
    for (int k = 0; k < K; ++k)
      check(slod_compute_error_norms(handle, (uint32_t)k, d_ell_fine + k * fine_size, nullptr, nullptr, nullptr, &ens_lod_norms[k], nullptr),
            "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_heat_ensemble(const unsigned int n_steps, const double dt, const double theta)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_heat_ensemble: assemble_mass_matrix_ensemble comes first");
    const int          K = (int)par.n_members;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_words = (std::size_t)n_patches * cap * spacedim * spacedim;
    if (!d_ens_shifted)
      d_ens_shifted = device_alloc<double>(n_words * K);
    double *d_u = device_alloc<double>(n_coarse * K);
    double *d_fine = device_alloc<double>(fine_size * K), *d_ell_fine = device_alloc<double>(fine_size * K);
    double *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    ensemble_elliptic_solutions(d_ell_fine);
    // S_k = M_k + theta dt A_k, one factor object, the loop
    check(slod_lod_matrix_combine_ensemble(handle, 1.0, d_ens_mass, (std::size_t)K, theta * dt, d_ens_values, (std::size_t)K, K,
                                           d_ens_shifted, (std::size_t)K, nullptr),
          "slod_lod_matrix_combine_ensemble");
    slod_lod_factor *f = nullptr;
    check(slod_lod_factor_create_ensemble(handle, d_ens_shifted, (std::size_t)K, K, d_ens_cols, nullptr, &f),
          "slod_lod_factor_create_ensemble");
    factors.push_back(f);
    check(slod_lod_factor_get_info(f, &lod_factor_info), "slod_lod_factor_get_info");
    if (hipMemset(d_u, 0, n_coarse * K * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_heat_ensemble: clearing the initial state failed");
    ens_heat_error.assign((std::size_t)n_steps * K, slod_error_norms{});
    source_open(n_steps + 1, (unsigned int)K, true);
    record_open(n_steps, (unsigned int)K, false, true);
    record_state(0, d_u, nullptr);
    for (unsigned int step = 0; step < n_steps; ++step)
      {
        source_arm(step);
        check(slod_lod_theta_steps_ensemble_direct(handle, f, d_ens_values, (std::size_t)K, d_ens_cols, dt, theta, 1, K, d_u,
                                                   (std::size_t)K, own_load(d_ens_rhs), (std::size_t)K, 0),
              "slod_lod_theta_steps_ensemble_direct");
        record_state(step + 1, d_u, nullptr);
        check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, d_u, (std::size_t)K, d_fine, fine_size,
                                            nullptr),
              "slod_lod_reconstruct_ensemble");
        for (int k = 0; k < K; ++k)
          check(slod_compute_error_norms(handle, (uint32_t)k, d_ell_fine + k * fine_size, d_fine + k * fine_size, nullptr, nullptr,
                                         &ens_heat_error[(std::size_t)step * K + k], nullptr),
                "slod_compute_error_norms");
      }
    record_close();
    drive_open = false;
    ensemble_moment_norms(d_fine, d_mean, d_var, ens_heat_mean_norms, ens_heat_dev_norms);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_wave_ensemble(const unsigned int n_steps, const double dt, const double beta, const double gamma)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_wave_ensemble: assemble_mass_matrix_ensemble comes first");
    const int          K = (int)par.n_members;
    const std::size_t  ld = (std::size_t)K;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_words = (std::size_t)n_patches * cap * spacedim * spacedim;
    if (!d_ens_sym)
      d_ens_sym = device_alloc<double>(n_words * K);
    if (!d_ens_shifted)
      d_ens_shifted = device_alloc<double>(n_words * K);
    double *d_state = device_alloc<double>(3 * n_coarse * K), *d_u = d_state, *d_v = d_u + n_coarse * K, *d_a = d_v + n_coarse * K;
    double *d_fine = device_alloc<double>(fine_size * K), *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    check(slod_lod_matrix_symmetrize_ensemble(handle, d_ens_values, ld, d_ens_cols, K, d_ens_sym, ld, nullptr),
          "slod_lod_matrix_symmetrize_ensemble");
    if (hipMemset(d_state, 0, 3 * n_coarse * K * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_wave_ensemble: clearing the initial state failed");
    std::vector<double> b(n_coarse * K), u(n_coarse * K);
    if (hipMemcpy(b.data(), d_ens_rhs, b.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("solve_wave_ensemble: download of the loads failed");
    if (load_quiet)
      b.assign(b.size(), 0.0);
    source_open(n_steps + 1, (unsigned int)K, true);
    const double *d_b0 = source_load(own_load(d_ens_rhs), drive_open ? device_alloc<double>(n_coarse * K) : nullptr);
    // the factors of M for the initial acceleration, then those of S = M + beta dt^2 A (no damping) for every step
    slod_lod_factor *f_M = nullptr, *f_S = nullptr;
    check(slod_lod_factor_create_ensemble(handle, d_ens_mass, ld, K, d_ens_cols, nullptr, &f_M), "slod_lod_factor_create_ensemble");
    factors.push_back(f_M);
    check(slod_lod_newmark_accel_ensemble_direct(handle, f_M, d_ens_sym, ld, d_ens_mass, ld, d_ens_cols, 0.0, 0.0, K, d_u, ld, d_v, ld,
                                                 d_b0, ld, d_a, ld),
          "slod_lod_newmark_accel_ensemble_direct");
    check(slod_lod_matrix_combine_ensemble(handle, 1.0, d_ens_mass, ld, beta * dt * dt, d_ens_sym, ld, K, d_ens_shifted, ld, nullptr),
          "slod_lod_matrix_combine_ensemble");
    check(slod_lod_factor_create_ensemble(handle, d_ens_shifted, ld, K, d_ens_cols, nullptr, &f_S), "slod_lod_factor_create_ensemble");
    factors.push_back(f_S);
    check(slod_lod_factor_get_info(f_S, &lod_factor_info), "slod_lod_factor_get_info");
    ens_wave_kinetic.assign((std::size_t)(n_steps + 1) * K, 0.0);
    ens_wave_potential.assign((std::size_t)(n_steps + 1) * K, 0.0);
    ens_wave_work.assign((std::size_t)(n_steps + 1) * K, 0.0);
    std::vector<double> kinetic(2 * ld), potential(2 * ld);
    record_open(n_steps, (unsigned int)K, true, true);
    record_state(0, d_u, d_v);
    for (unsigned int step = 0; step < n_steps; ++step)
      {
        source_arm(step);
        check(slod_lod_newmark_steps_ensemble_direct(handle, f_S, d_ens_sym, ld, d_ens_mass, ld, d_ens_cols, dt, beta, gamma, 0.0, 0.0, 1,
                                                     K, d_u, ld, d_v, ld, d_a, ld, own_load(d_ens_rhs), ld, 0, kinetic.data(),
                                                     potential.data()),
              "slod_lod_newmark_steps_ensemble_direct");
        record_state(step + 1, d_u, d_v);
        if (hipMemcpy(u.data(), d_u, u.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          throw std::runtime_error("solve_wave_ensemble: download of the states failed");
        for (int k = 0; k < K; ++k)
          {
            if (step == 0)
              {
                ens_wave_kinetic[k]   = kinetic[k];
                ens_wave_potential[k] = potential[k];
              }
            ens_wave_kinetic[(std::size_t)(step + 1) * K + k]   = kinetic[ld + k];
            ens_wave_potential[(std::size_t)(step + 1) * K + k] = potential[ld + k];
            double work = 0.0;
            for (std::size_t i = 0; i < n_coarse; ++i)
              work += u[i * K + k] * b[i * K + k];
            ens_wave_work[(std::size_t)(step + 1) * K + k] = work;
          }
      }
    check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, d_u, ld, d_fine, fine_size, nullptr),
          "slod_lod_reconstruct_ensemble");
    record_close();
    drive_open = false;
    ensemble_moment_norms(d_fine, d_mean, d_var, ens_wave_mean_norms, ens_wave_dev_norms);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_harmonic_ensemble(const std::vector<double> &omegas, const double damp_mass, const double damp_stiff)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_harmonic_ensemble: assemble_mass_matrix_ensemble comes first");
    if (omegas.empty())
      throw std::runtime_error("solve_harmonic_ensemble: no frequency");
    const int          K = (int)par.n_members;
    const std::size_t  F = omegas.size(), ld_m = (std::size_t)K, ld = F * K;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_words = (std::size_t)n_patches * cap * spacedim * spacedim;
    if (!d_ens_sym)
      d_ens_sym = device_alloc<double>(n_words * K);
    // the response interleaved [row][frequency][member], as the call writes it
    double *d_ur = device_alloc<double>(2 * n_coarse * ld), *d_ui = d_ur + n_coarse * ld;
    double *d_fine = device_alloc<double>(fine_size * K), *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    check(slod_lod_matrix_symmetrize_ensemble(handle, d_ens_values, ld_m, d_ens_cols, K, d_ens_sym, ld_m, nullptr),
          "slod_lod_matrix_symmetrize_ensemble");
    ens_harmonic_growth.assign(ld, 0.0);
    ens_harmonic_residuals.assign(ld, 0.0);
    ens_harmonic_quantities.assign(4 * ld, 0.0);
    // d_ens_rhs: the loads C_k^T f of solve_ensemble() (slod_lod_rhs_ensemble, f = 1), column = member
    check(slod_lod_harmonic_response_ensemble(handle, d_ens_sym, ld_m, d_ens_mass, ld_m, d_ens_cols, K, damp_mass, damp_stiff,
                                              omegas.data(), (int)F, d_ens_rhs, nullptr, ld_m, 1, d_ur, d_ui, ld,
                                              ens_harmonic_residuals.data(), ens_harmonic_growth.data(), ens_harmonic_quantities.data()),
          "slod_lod_harmonic_response_ensemble");
    // u^H M u and u^H A u as solve_harmonic forms them (the two planes add), on every frequency's block of K columns
    ens_harmonic_amplitude.assign(ld, 0.0);
    ens_harmonic_power.assign(ld, 0.0);
    std::vector<double> q[4] = {std::vector<double>(K), std::vector<double>(K), std::vector<double>(K), std::vector<double>(K)};
    double              best = -1.0;
    for (std::size_t k = 0; k < F; ++k)
      {
        const double *ur = d_ur + k * K, *ui = d_ui + k * K;
        check(slod_lod_inner_ensemble(handle, d_ens_mass, ld_m, d_ens_cols, ur, ld, ur, ld, K, q[0].data(), nullptr), "slod_lod_inner_ensemble");
        check(slod_lod_inner_ensemble(handle, d_ens_mass, ld_m, d_ens_cols, ui, ld, ui, ld, K, q[1].data(), nullptr), "slod_lod_inner_ensemble");
        check(slod_lod_inner_ensemble(handle, d_ens_sym, ld_m, d_ens_cols, ur, ld, ur, ld, K, q[2].data(), nullptr), "slod_lod_inner_ensemble");
        check(slod_lod_inner_ensemble(handle, d_ens_sym, ld_m, d_ens_cols, ui, ld, ui, ld, K, q[3].data(), nullptr), "slod_lod_inner_ensemble");
        double mean = 0.0;
        for (int m = 0; m < K; ++m)
          {
            const double uMu = q[0][m] + q[1][m], uAu = q[2][m] + q[3][m];
            ens_harmonic_amplitude[k * K + m] = std::sqrt(uMu);
            ens_harmonic_power[k * K + m]     = 0.5 * omegas[k] * (damp_mass * uMu + damp_stiff * uAu);
            mean += ens_harmonic_amplitude[k * K + m];
          }
        if (mean / K > best)
          best = mean / K, ens_harmonic_peak = (unsigned int)k;
      }
    // the two planes of the loudest frequency on the fine grid, and their moments over the members
    for (int part = 0; part < 2; ++part)
      {
        const double *block = (part == 0 ? d_ur : d_ui) + (std::size_t)ens_harmonic_peak * K;
        check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, block, ld, d_fine, fine_size, nullptr),
              "slod_lod_reconstruct_ensemble");
        ensemble_moment_norms(d_fine, d_mean, d_var, ens_harmonic_norms[2 * part], ens_harmonic_norms[2 * part + 1]);
      }
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_eigenproblem_ensemble(const unsigned int n_eig, const double sigma)
  {
    eigenproblem_ensemble(n_eig, sigma, false, false);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_eigenproblem_ensemble_near(const double sigma, const unsigned int n_eig, const bool ldl)
  {
    eigenproblem_ensemble(n_eig, sigma, true, ldl);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::eigenproblem_ensemble(const unsigned int n_eig, const double sigma, const bool near, const bool ldl)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_eigenproblem_ensemble: assemble_mass_matrix_ensemble comes first");
    const int          K = (int)par.n_members;
    const std::size_t  ld = (std::size_t)K;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  n_coarse = (std::size_t)n_patches * spacedim;
    if (n_eig < 1 || n_eig > n_coarse || n_eig > 64)
      throw std::runtime_error("solve_eigenproblem_ensemble: n_eig outside 1 .. min(64, unknowns)");
    const int cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_words = (std::size_t)n_patches * cap * spacedim * spacedim;
    // the defaults of solve_eigenproblem
    const int n_block = (int)std::min(std::min<std::size_t>(64, n_coarse), n_eig + std::max<std::size_t>(4, n_eig / 2));
    const int max_outer = 200;
    if (!d_ens_sym)
      d_ens_sym = device_alloc<double>(n_words * K);
    double *d_x = device_alloc<double>(n_coarse * n_block * K);
    check(slod_lod_matrix_symmetrize_ensemble(handle, d_ens_values, ld, d_ens_cols, K, d_ens_sym, ld, nullptr),
          "slod_lod_matrix_symmetrize_ensemble");
    const double *d_S = d_ens_sym;
    if (sigma != 0.0)
      {
        if (!d_ens_shifted)
          d_ens_shifted = device_alloc<double>(n_words * K);
        check(slod_lod_matrix_combine_ensemble(handle, 1.0, d_ens_sym, ld, -sigma, d_ens_mass, ld, K, d_ens_shifted, ld, nullptr),
              "slod_lod_matrix_combine_ensemble");
        d_S = d_ens_shifted;
      }
    slod_lod_factor *f = nullptr;
    if (ldl)
      check(slod_lod_factor_create_ldl_ensemble(handle, d_S, ld, K, d_ens_cols, nullptr, &f), "slod_lod_factor_create_ldl_ensemble");
    else
      check(slod_lod_factor_create_ensemble(handle, d_S, ld, K, d_ens_cols, nullptr, &f), "slod_lod_factor_create_ensemble");
    factors.push_back(f);
    check(slod_lod_factor_get_info(f, &lod_factor_info), "slod_lod_factor_get_info");
    ens_factor_inertia.assign(ldl ? K : 0, slod_lod_factor_inertia_info{});
    for (int k = 0; k < (ldl ? K : 0); ++k)
      check(slod_lod_factor_inertia(f, k, &ens_factor_inertia[k]), "slod_lod_factor_inertia");
    ens_eig_block = n_block;
    ens_eigenvalues.assign((std::size_t)K * n_block, 0.0);
    ens_eig_residuals.assign((std::size_t)K * n_block, 0.0);
    ens_eig_outer.assign(K, 0);
    const int rc =
      near ? slod_lod_eigs_shift_ensemble_direct(handle, f, sigma, d_ens_sym, ld, d_ens_mass, ld, d_ens_cols, K, (int)n_eig, n_block, 0,
                                                 d_x, ld * n_block, 1e-10, max_outer, ens_eigenvalues.data(),
                                                 ens_eig_residuals.data(), ens_eig_outer.data()) :
             slod_lod_eigs_ensemble_direct(handle, f, d_ens_sym, ld, d_ens_mass, ld, d_ens_cols, K, (int)n_eig, n_block, 0, d_x,
                                           ld * n_block, 1e-10, max_outer, ens_eigenvalues.data(), ens_eig_residuals.data(),
                                           ens_eig_outer.data());
    check(rc < 0 ? rc : 0, near ? "slod_lod_eigs_shift_ensemble_direct" : "slod_lod_eigs_ensemble_direct");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_mass_matrix()
  {
    if (!d_lod_values)
      throw std::runtime_error("assemble_mass_matrix: assemble_global_matrix comes first");
    const unsigned int n_patches = (unsigned int)patches.size();
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_slots = (std::size_t)n_patches * cap;
    if (!d_lod_mass)
      d_lod_mass = device_alloc<double>(n_slots * spacedim * spacedim);
    // the call writes its columns; they must be those of A_LOD, which the solves use for both matrices
    uint32_t *d_m_cols = nullptr;
    if (hipMalloc((void **)&d_m_cols, n_slots * sizeof(uint32_t)) != hipSuccess)
      throw std::runtime_error("assemble_mass_matrix: hipMalloc of the columns failed");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    const int             rc = slod_lod_mass_matrix(handle, rows.data(), n_patches, d_basis, basis_stride, nullptr, d_lod_mass,
                                                    d_m_cols, nullptr);
    std::vector<uint32_t> m_cols(n_slots), a_cols(n_slots);
    const bool            copied = rc == SLOD_OK &&
                        hipMemcpy(m_cols.data(), d_m_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                        hipMemcpy(a_cols.data(), d_lod_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_m_cols);
    check(rc, "slod_lod_mass_matrix");
    if (!copied || m_cols != a_cols)
      throw std::runtime_error("assemble_mass_matrix: the pattern of M_LOD differs from that of A_LOD");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_damping_matrix(const std::vector<double> &sigma)
  {
    if (!d_lod_values)
      throw std::runtime_error("assemble_damping_matrix: assemble_global_matrix comes first");
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    if (sigma.size() != NE * NE)
      throw std::runtime_error("assemble_damping_matrix: sigma has one value per fine element");
    const int cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    const std::size_t n_slots = (std::size_t)n_patches * cap, n_values = n_slots * spacedim * spacedim;
    if (!d_lod_damping)
      d_lod_damping = device_alloc<double>(n_values);
    double *d_sigma = device_alloc<double>(sigma.size());
    if (hipMemcpy(d_sigma, sigma.data(), sigma.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("assemble_damping_matrix: upload of sigma failed");
    uint32_t *d_m_cols = nullptr;
    if (hipMalloc((void **)&d_m_cols, n_slots * sizeof(uint32_t)) != hipSuccess)
      throw std::runtime_error("assemble_damping_matrix: hipMalloc of the columns failed");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    const int             rc = slod_lod_mass_matrix(handle, rows.data(), n_patches, d_basis, basis_stride, d_sigma, d_lod_damping,
                                                    d_m_cols, nullptr);
    std::vector<uint32_t> m_cols(n_slots), a_cols(n_slots);
    std::vector<double>   values(n_values);
    const bool            copied = rc == SLOD_OK &&
                        hipMemcpy(m_cols.data(), d_m_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                        hipMemcpy(a_cols.data(), d_lod_cols, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                        hipMemcpy(values.data(), d_lod_damping, n_values * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_m_cols);
    check(rc, "slod_lod_mass_matrix");
    if (!copied || m_cols != a_cols)
      throw std::runtime_error("assemble_damping_matrix: the pattern of D_LOD differs from that of A_LOD");
    lod_damping_zero_rows = 0;
    for (unsigned int p = 0; p < n_patches; ++p)
      for (int d = 0; d < spacedim; ++d)
        {
          bool zero = true;
          for (int j = 0; j < cap; ++j)
            if (a_cols[(std::size_t)p * cap + j] < n_patches)
              for (int e = 0; e < spacedim; ++e)
                zero = zero && values[((std::size_t)p * cap + j) * spacedim * spacedim + d * spacedim + e] == 0.0;
          lod_damping_zero_rows += zero;
        }
  }

  template <int dim, int spacedim>
  slod_lod_factor *LOD<dim, spacedim>::factor_lod_matrix(const double *d_values, const bool ldl)
  {
    slod_lod_factor *f = nullptr;
    if (ldl)
      check(slod_lod_factor_create_ldl(handle, d_values, d_lod_cols, &f), "slod_lod_factor_create_ldl");
    else
      check(slod_lod_factor_create(handle, d_values, d_lod_cols, &f), "slod_lod_factor_create");
    factors.push_back(f);
    check(slod_lod_factor_get_info(f, &lod_factor_info), "slod_lod_factor_get_info");
    if (ldl)
      check(slod_lod_factor_inertia(f, 0, &lod_factor_inertia), "slod_lod_factor_inertia");
    return f;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_heat(const unsigned int n_steps, const double dt, const double theta, const bool direct)
  {
    if (!d_lod_mass || !d_fem_rhs)
      throw std::runtime_error("solve_heat: assemble_mass_matrix and assemble_and_solve_fem_problem come first");
    const unsigned int    n_patches = (unsigned int)patches.size();
    const std::size_t     n_coarse = (std::size_t)n_patches * spacedim;
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    // allocated on the first call, re-used by later ones
    if (!d_heat_rhs)
      d_heat_rhs = device_alloc<double>(n_coarse);
    if (!d_heat_u)
      d_heat_u = device_alloc<double>(n_coarse);
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_heat_rhs, nullptr), "slod_lod_rhs");
    if (hipMemset(d_heat_u, 0, n_coarse * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_heat: clearing the initial state failed");
    lod_heat_iterations.assign(n_steps, 0);
    lod_heat_residuals.assign(n_steps, 0.0);
    if (direct)
      {
        // S = M + theta dt A_LOD with the coefficients of slod_lod_theta_steps; the factor reads its lower triangle
        const int cap = slod_lod_row_capacity(handle);
        check(cap, "slod_lod_row_capacity");
        if (!d_lod_shifted)
          d_lod_shifted = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
        check(slod_lod_matrix_combine(handle, 1.0, d_lod_mass, theta * dt, d_lod_values, d_lod_shifted, nullptr),
              "slod_lod_matrix_combine");
        if (hipDeviceSynchronize() != hipSuccess)
          throw std::runtime_error("solve_heat: forming S failed");
        slod_lod_factor *f = factor_lod_matrix(d_lod_shifted);
        source_open(n_steps + 1, 1, false);
        record_open(n_steps, 1, false, false);
        record_arm(n_steps);
        source_arm(0);
        check(slod_lod_theta_steps_direct(handle, f, d_lod_values, d_lod_cols, dt, theta, (int)n_steps, 1, d_heat_u, 1,
                                          own_load(d_heat_rhs), 1, 0),
              "slod_lod_theta_steps_direct");
        record_close();
        drive_open = false;
        return;
      }
    source_open(n_steps + 1, 1, false);
    record_open(n_steps, 1, false, false);
    record_arm(n_steps);
    source_arm(0);
    check(slod_lod_theta_steps(handle, d_lod_values, d_lod_mass, d_lod_cols, dt, theta, (int)n_steps, 1, d_heat_u, 1, own_load(d_heat_rhs), 1,
                               0, lod_rel_tol, lod_max_iterations, lod_heat_iterations.data(), lod_heat_residuals.data()),
          "slod_lod_theta_steps");
    record_close();
    drive_open = false;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::compare_heat_with_lod()
  {
    if (!d_heat_u || !d_lod_u)
      throw std::runtime_error("compare_heat_with_lod: solve and solve_heat come first");
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t fine_size = (NE + 1) * (NE + 1) * spacedim;
    if (!d_heat_fine)
      d_heat_fine = device_alloc<double>(2 * fine_size); // the elliptic and the heat state, re-used by later calls
    double *d_lod_fine = d_heat_fine + fine_size;
    check(slod_lod_reconstruct(handle, d_basis, basis_stride, d_lod_u, d_lod_fine, nullptr), "slod_lod_reconstruct");
    check(slod_lod_reconstruct(handle, d_basis, basis_stride, d_heat_u, d_heat_fine, nullptr), "slod_lod_reconstruct");
    check(slod_compute_error_norms(handle, 0, d_lod_fine, d_heat_fine, nullptr, nullptr, &heat_lod_error, nullptr),
          "slod_compute_error_norms");
    check(slod_compute_error_norms(handle, 0, d_lod_fine, nullptr, nullptr, nullptr, &lod_norms, nullptr),
          "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_eigenproblem(const unsigned int n_eig, const bool direct, const double sigma)
  {
    eigenproblem(n_eig, direct, sigma, false, false);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_eigenproblem_near(const double sigma, const unsigned int n_eig, const bool ldl)
  {
    eigenproblem(n_eig, true, sigma, true, ldl);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::eigenproblem(const unsigned int n_eig, const bool direct, const double sigma, const bool near,
                                        const bool ldl)
  {
    if (!d_lod_mass)
      throw std::runtime_error("solve_eigenproblem: assemble_global_matrix and assemble_mass_matrix come first");
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  n_coarse = (std::size_t)n_patches * spacedim;
    if (n_eig < 1 || n_eig > n_coarse || n_eig > 64)
      throw std::runtime_error("solve_eigenproblem: n_eig outside 1 .. min(64, unknowns)");
    const std::size_t NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t fine_size = (NE + 1) * (NE + 1) * spacedim;
    const int         cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    // the defaults of the Python binding
    const int n_block = (int)std::min(std::min<std::size_t>(64, n_coarse), n_eig + std::max<std::size_t>(4, n_eig / 2));
    const int max_outer = 200;
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    d_eig_x    = device_alloc<double>(n_coarse * n_block);
    d_eig_fine = device_alloc<double>(n_eig * fine_size);
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    lod_eigenvalues.assign(n_block, 0.0);
    lod_eig_residuals.assign(n_block, 0.0);
    lod_eig_inner_iterations.assign(max_outer, 0);
    int outer;
    if (direct)
      {
        // S = sym(A_LOD) - sigma M_LOD; sigma = 0: the factor of sym(A_LOD) itself
        const double *d_S = d_lod_sym;
        if (sigma != 0.0)
          {
            if (!d_lod_shifted)
              d_lod_shifted = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
            check(slod_lod_matrix_combine(handle, 1.0, d_lod_sym, -sigma, d_lod_mass, d_lod_shifted, nullptr), "slod_lod_matrix_combine");
            d_S = d_lod_shifted;
          }
        if (hipDeviceSynchronize() != hipSuccess)
          throw std::runtime_error("solve_eigenproblem: forming S failed");
        slod_lod_factor *f = factor_lod_matrix(d_S, ldl);
        outer = near ? slod_lod_eigs_shift_direct(handle, f, sigma, d_lod_sym, d_lod_mass, d_lod_cols, (int)n_eig, n_block, 0, d_eig_x,
                                                  (std::size_t)n_block, 1e-10, max_outer, lod_eigenvalues.data(),
                                                  lod_eig_residuals.data()) :
                       slod_lod_eigs_direct(handle, f, d_lod_sym, d_lod_mass, d_lod_cols, (int)n_eig, n_block, 0, d_eig_x,
                                            (std::size_t)n_block, 1e-10, max_outer, lod_eigenvalues.data(), lod_eig_residuals.data());
        check(outer < 0 ? outer : 0, near ? "slod_lod_eigs_shift_direct" : "slod_lod_eigs_direct");
        lod_eig_inner_iterations.clear();
      }
    else
      {
        outer = slod_lod_eigs(handle, d_lod_sym, d_lod_mass, d_lod_cols, (int)n_eig, n_block, 0, d_eig_x, (std::size_t)n_block, 1e-10,
                              max_outer, 1e-12, 2000, lod_eigenvalues.data(), lod_eig_residuals.data(),
                              lod_eig_inner_iterations.data());
        check(outer < 0 ? outer : 0, "slod_lod_eigs");
        lod_eig_inner_iterations.resize(outer);
      }
    lod_eig_outer = outer;
    check(slod_lod_reconstruct_multi(handle, d_basis, basis_stride, d_eig_x, (std::size_t)n_block, (int)n_eig, d_eig_fine, fine_size,
                                     nullptr),
          "slod_lod_reconstruct_multi");
    lod_eig_norms.assign(n_eig, slod_error_norms{});
    for (unsigned int k = 0; k < n_eig; ++k)
      check(slod_compute_error_norms(handle, 0, d_eig_fine + k * fine_size, nullptr, nullptr, nullptr, &lod_eig_norms[k], nullptr),
            "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_harmonic(const std::vector<double> &omegas, const double damp_mass, const double damp_stiff)
  {
    if (!d_lod_mass || !d_fem_rhs)
      throw std::runtime_error("solve_harmonic: assemble_mass_matrix and assemble_and_solve_fem_problem come first");
    if (omegas.empty())
      throw std::runtime_error("solve_harmonic: no frequency");
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  n_coarse = (std::size_t)n_patches * spacedim, K = omegas.size();
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    if (harmonic_capacity < K) // (an earlier, smaller buffer stays with the object until it is destroyed)
      {
        d_harmonic        = device_alloc<double>((1 + 2 * K) * n_coarse);
        harmonic_capacity = K;
      }
    // the response interleaved [row][frequency], as the call writes it
    double *d_b = d_harmonic, *d_ur = d_b + n_coarse, *d_ui = d_ur + K * n_coarse;
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_b, nullptr), "slod_lod_rhs");
    lod_harmonic_growth.assign(K, 0.0);
    lod_harmonic_residuals.assign(K, 0.0);
    lod_harmonic_amplitude.assign(K, 0.0);
    lod_harmonic_power.assign(K, 0.0);
    if (d_lod_damping) // the sponge: S gains i omega D, and the call returns u^H M u, u^H A u and u^H D u
      {
        std::vector<double> quantities(5 * K);
        check(slod_lod_harmonic_response_damped(handle, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, damp_mass, damp_stiff,
                                                omegas.data(), (int)K, d_b, nullptr, 1, 1, d_ur, d_ui, K, lod_harmonic_residuals.data(),
                                                lod_harmonic_growth.data(), quantities.data()),
              "slod_lod_harmonic_response_damped");
        for (std::size_t k = 0; k < K; ++k)
          {
            const double *q = quantities.data() + 5 * k;
            lod_harmonic_amplitude[k] = std::sqrt(q[0]);
            lod_harmonic_power[k]     = 0.5 * omegas[k] * (damp_mass * q[0] + damp_stiff * q[1] + q[2]);
          }
        return;
      }
    check(slod_lod_harmonic_response(handle, d_lod_sym, d_lod_mass, d_lod_cols, damp_mass, damp_stiff, omegas.data(), (int)K, d_b,
                                     nullptr, 1, 1, d_ur, d_ui, K, lod_harmonic_residuals.data(), lod_harmonic_growth.data()),
          "slod_lod_harmonic_response");
    // u^H M u and u^H A u: the two planes add
    std::vector<double> q[4] = {std::vector<double>(K), std::vector<double>(K), std::vector<double>(K), std::vector<double>(K)};
    check(slod_lod_inner_multi(handle, d_lod_mass, d_lod_cols, d_ur, K, d_ur, K, (int)K, q[0].data(), nullptr), "slod_lod_inner_multi");
    check(slod_lod_inner_multi(handle, d_lod_mass, d_lod_cols, d_ui, K, d_ui, K, (int)K, q[1].data(), nullptr), "slod_lod_inner_multi");
    check(slod_lod_inner_multi(handle, d_lod_sym, d_lod_cols, d_ur, K, d_ur, K, (int)K, q[2].data(), nullptr), "slod_lod_inner_multi");
    check(slod_lod_inner_multi(handle, d_lod_sym, d_lod_cols, d_ui, K, d_ui, K, (int)K, q[3].data(), nullptr), "slod_lod_inner_multi");
    for (std::size_t k = 0; k < K; ++k)
      {
        const double uMu = q[0][k] + q[1][k], uAu = q[2][k] + q[3][k];
        lod_harmonic_amplitude[k] = std::sqrt(uMu);
        lod_harmonic_power[k]     = 0.5 * omegas[k] * (damp_mass * uMu + damp_stiff * uAu);
      }
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_wave(const unsigned int n_steps, const double dt, const double beta, const double gamma,
                                      const bool direct)
  {
    if (!d_lod_mass || !d_fem_rhs)
      throw std::runtime_error("solve_wave: assemble_mass_matrix and assemble_and_solve_fem_problem come first");
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  n_coarse = (std::size_t)n_patches * spacedim;
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    // allocated on the first call, re-used by later ones
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    if (!d_wave_state)
      d_wave_state = device_alloc<double>(4 * n_coarse);
    if (!d_wave_fine)
      d_wave_fine = device_alloc<double>(fine_size);
    double *d_u = d_wave_state, *d_v = d_u + n_coarse, *d_a = d_v + n_coarse, *d_b = d_a + n_coarse;
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_b, nullptr), "slod_lod_rhs");
    if (hipMemset(d_wave_state, 0, 3 * n_coarse * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_wave: clearing the initial state failed");
    std::vector<double> b(n_coarse), u(n_coarse);
    if (hipMemcpy(b.data(), d_b, n_coarse * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("solve_wave: download of the load failed");
    if (load_quiet)
      b.assign(n_coarse, 0.0);
    source_open(n_steps + 1, 1, false);
    if (drive_open && !d_wave_load0)
      d_wave_load0 = device_alloc<double>(n_coarse);
    const double *d_b0 = source_load(own_load(d_b), d_wave_load0); // b^0 of the initial acceleration
    slod_lod_factor *f_S = nullptr;
    if (direct)
      {
        // the factor of M for the initial acceleration, then that of S = M + beta dt^2 A (no damping) for every step
        // (with a sponge D the _damped calls; without one they are the calls they extend)
        check(slod_lod_newmark_accel_damped_direct(handle, factor_lod_matrix(d_lod_mass), d_lod_sym, d_lod_mass, d_lod_damping,
                                                   d_lod_cols, 0.0, 0.0, 1, d_u, 1, d_v, 1, d_b0, 1, d_a, 1),
              "slod_lod_newmark_accel_damped_direct");
        if (!d_lod_shifted)
          d_lod_shifted = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
        check(slod_lod_matrix_combine(handle, 1.0, d_lod_mass, beta * dt * dt, d_lod_sym, d_lod_shifted, nullptr),
              "slod_lod_matrix_combine");
        if (d_lod_damping) // S + gamma dt D, the second rounding of the CG call
          check(slod_lod_matrix_combine(handle, 1.0, d_lod_shifted, gamma * dt, d_lod_damping, d_lod_shifted, nullptr),
                "slod_lod_matrix_combine");
        if (hipDeviceSynchronize() != hipSuccess)
          throw std::runtime_error("solve_wave: forming S failed");
        f_S = factor_lod_matrix(d_lod_shifted);
      }
    else
      {
        const int rc = slod_lod_newmark_accel_damped(handle, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, 0.0, 0.0, 1, d_u, 1, d_v,
                                                     1, d_b0, 1, d_a, 1, lod_rel_tol, lod_max_iterations, nullptr, nullptr);
        check(rc < 0 ? rc : 0, "slod_lod_newmark_accel_damped");
      }
    lod_wave_iterations.assign(n_steps, 0);
    lod_wave_residuals.assign(n_steps, 0.0);
    lod_wave_kinetic.assign(n_steps + 1, 0.0);
    lod_wave_potential.assign(n_steps + 1, 0.0);
    lod_wave_work.assign(n_steps + 1, 0.0);
    record_open(n_steps, 1, true, false);
    record_state(0, d_u, d_v);
    for (unsigned int k = 0; k < n_steps; ++k)
      {
        double    kinetic[2], potential[2];
        source_arm(k);
        if (direct)
          check(slod_lod_newmark_steps_damped_direct(handle, f_S, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, dt, beta, gamma, 0.0,
                                                     0.0, 1, 1, d_u, 1, d_v, 1, d_a, 1, own_load(d_b), 1, 0, kinetic, potential),
                "slod_lod_newmark_steps_damped_direct");
        else
          {
            const int its = slod_lod_newmark_steps_damped(handle, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, dt, beta, gamma, 0.0,
                                                          0.0, 1, 1, d_u, 1, d_v, 1, d_a, 1, own_load(d_b), 1, 0, lod_rel_tol,
                                                          lod_max_iterations, &lod_wave_iterations[k], &lod_wave_residuals[k], kinetic,
                                                          potential);
            check(its < 0 ? its : 0, "slod_lod_newmark_steps_damped");
          }
        record_state(k + 1, d_u, d_v);
        if (hipMemcpy(u.data(), d_u, n_coarse * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          throw std::runtime_error("solve_wave: download of the state failed");
        if (k == 0)
          {
            lod_wave_kinetic[0]   = kinetic[0];
            lod_wave_potential[0] = potential[0];
          }
        lod_wave_kinetic[k + 1]   = kinetic[1];
        lod_wave_potential[k + 1] = potential[1];
        double work = 0.0;
        for (std::size_t i = 0; i < n_coarse; ++i)
          work += u[i] * b[i];
        lod_wave_work[k + 1] = work;
      }
    record_close();
    drive_open = false;
    check(slod_lod_reconstruct(handle, d_basis, basis_stride, d_u, d_wave_fine, nullptr), "slod_lod_reconstruct");
    check(slod_compute_error_norms(handle, 0, d_wave_fine, nullptr, nullptr, nullptr, &wave_norms, nullptr),
          "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  slod_lod_factor *LOD<dim, spacedim>::factor_lod_irk(const int scheme, const int order, const double dt)
  {
    double alpha[2], beta[2];
    if (slod_lod_irk_coefficients(scheme, order, dt, 0.0, 0.0, alpha, beta) != SLOD_OK)
      throw std::runtime_error(std::string("slod_lod_irk_coefficients: ") + slod_last_error(nullptr));
    slod_lod_factor *f = nullptr;
    if (d_lod_damping && order == 2) // the sponge: S + z D
      {
        double z[2];
        if (slod_lod_irk_damping_coefficient(scheme, dt, z) != SLOD_OK)
          throw std::runtime_error(std::string("slod_lod_irk_damping_coefficient: ") + slod_last_error(nullptr));
        check(slod_lod_factor_create_zldl3(handle, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, alpha, beta, z, 1, nullptr, &f),
              "slod_lod_factor_create_zldl3");
      }
    else
      check(slod_lod_factor_create_zldl(handle, d_lod_sym, d_lod_mass, d_lod_cols, alpha, beta, 1, nullptr, &f),
            "slod_lod_factor_create_zldl");
    factors.push_back(f);
    check(slod_lod_factor_get_info(f, &lod_factor_info), "slod_lod_factor_get_info");
    check(slod_lod_factor_inertia(f, 0, &lod_factor_inertia), "slod_lod_factor_inertia");
    return f;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_heat_irk(const int scheme, const unsigned int n_steps, const double dt)
  {
    if (!d_lod_mass || !d_fem_rhs)
      throw std::runtime_error("solve_heat_irk: assemble_mass_matrix and assemble_and_solve_fem_problem come first");
    const unsigned int    n_patches = (unsigned int)patches.size();
    const std::size_t     n_coarse = (std::size_t)n_patches * spacedim;
    const int             cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    if (!d_heat_rhs)
      d_heat_rhs = device_alloc<double>(n_coarse);
    if (!d_heat_u)
      d_heat_u = device_alloc<double>(n_coarse);
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_heat_rhs, nullptr), "slod_lod_rhs");
    if (hipMemset(d_heat_u, 0, n_coarse * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_heat_irk: clearing the initial state failed");
    lod_heat_iterations.assign(n_steps, 0);
    lod_heat_residuals.assign(n_steps, 0.0);
    slod_lod_factor *f = factor_lod_irk(scheme, 1, dt);
    source_open(2 * n_steps, 1, false);
    record_open(n_steps, 1, false, false);
    record_arm(n_steps);
    source_arm(0);
    check(slod_lod_irk_heat_steps_direct(handle, f, 0, scheme, d_lod_sym, d_lod_cols, dt, (int)n_steps, 1, d_heat_u, 1,
                                         own_load(d_heat_rhs), 1, 0),
          "slod_lod_irk_heat_steps_direct");
    record_close();
    drive_open = false;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_wave_irk(const int scheme, const unsigned int n_steps, const double dt)
  {
    if (!d_lod_mass || !d_fem_rhs)
      throw std::runtime_error("solve_wave_irk: assemble_mass_matrix and assemble_and_solve_fem_problem come first");
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  n_coarse = (std::size_t)n_patches * spacedim;
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim;
    const int          cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    std::vector<uint32_t> rows(n_patches);
    for (unsigned int p = 0; p < n_patches; ++p)
      rows[p] = p;
    if (!d_lod_sym)
      d_lod_sym = device_alloc<double>((std::size_t)n_patches * cap * spacedim * spacedim);
    if (!d_wave_state)
      d_wave_state = device_alloc<double>(4 * n_coarse);
    if (!d_wave_fine)
      d_wave_fine = device_alloc<double>(fine_size);
    double *d_u = d_wave_state, *d_v = d_u + n_coarse, *d_b = d_v + 2 * n_coarse;
    check(slod_lod_matrix_symmetrize(handle, d_lod_values, d_lod_cols, d_lod_sym, nullptr), "slod_lod_matrix_symmetrize");
    check(slod_lod_rhs(handle, rows.data(), n_patches, d_basis, basis_stride, d_fem_rhs, d_b, nullptr), "slod_lod_rhs");
    if (hipMemset(d_wave_state, 0, 3 * n_coarse * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_wave_irk: clearing the initial state failed");
    std::vector<double> b(n_coarse), u(n_coarse);
    if (hipMemcpy(b.data(), d_b, n_coarse * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("solve_wave_irk: download of the load failed");
    if (load_quiet)
      b.assign(n_coarse, 0.0);
    source_open(2 * n_steps, 1, false);
    slod_lod_factor *f = factor_lod_irk(scheme, 2, dt);
    lod_wave_iterations.assign(n_steps, 0);
    lod_wave_residuals.assign(n_steps, 0.0);
    lod_wave_kinetic.assign(n_steps + 1, 0.0);
    lod_wave_potential.assign(n_steps + 1, 0.0);
    lod_wave_work.assign(n_steps + 1, 0.0);
    record_open(n_steps, 1, true, false);
    record_state(0, d_u, d_v);
    for (unsigned int k = 0; k < n_steps; ++k)
      {
        double kinetic[2], potential[2];
        source_arm(2 * k);
        check(slod_lod_irk_wave_steps_damped_direct(handle, f, 0, scheme, d_lod_sym, d_lod_mass, d_lod_damping, d_lod_cols, dt, 0.0, 0.0,
                                                    1, 1, d_u, 1, d_v, 1, own_load(d_b), 1, 0, kinetic, potential),
              "slod_lod_irk_wave_steps_damped_direct");
        record_state(k + 1, d_u, d_v);
        if (hipMemcpy(u.data(), d_u, n_coarse * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          throw std::runtime_error("solve_wave_irk: download of the state failed");
        if (k == 0)
          {
            lod_wave_kinetic[0]   = kinetic[0];
            lod_wave_potential[0] = potential[0];
          }
        lod_wave_kinetic[k + 1]   = kinetic[1];
        lod_wave_potential[k + 1] = potential[1];
        double work = 0.0;
        for (std::size_t i = 0; i < n_coarse; ++i)
          work += u[i] * b[i];
        lod_wave_work[k + 1] = work;
      }
    record_close();
    drive_open = false;
    check(slod_lod_reconstruct(handle, d_basis, basis_stride, d_u, d_wave_fine, nullptr), "slod_lod_reconstruct");
    check(slod_compute_error_norms(handle, 0, d_wave_fine, nullptr, nullptr, nullptr, &wave_norms, nullptr),
          "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  slod_lod_factor *LOD<dim, spacedim>::factor_lod_irk_ensemble(const int scheme, const int order, const double dt)
  {
    const int         K = (int)par.n_members;
    const std::size_t ld = (std::size_t)K;
    const int         cap = slod_lod_row_capacity(handle);
    check(cap, "slod_lod_row_capacity");
    if (!d_ens_sym)
      d_ens_sym = device_alloc<double>((std::size_t)patches.size() * cap * spacedim * spacedim * K);
    check(slod_lod_matrix_symmetrize_ensemble(handle, d_ens_values, ld, d_ens_cols, K, d_ens_sym, ld, nullptr),
          "slod_lod_matrix_symmetrize_ensemble");
    double alpha[2], beta[2];
    if (slod_lod_irk_coefficients(scheme, order, dt, 0.0, 0.0, alpha, beta) != SLOD_OK)
      throw std::runtime_error(std::string("slod_lod_irk_coefficients: ") + slod_last_error(nullptr));
    slod_lod_factor *f = nullptr;
    check(slod_lod_factor_create_zldl_ensemble(handle, d_ens_sym, ld, d_ens_mass, ld, K, d_ens_cols, alpha, beta, 1, nullptr, &f),
          "slod_lod_factor_create_zldl_ensemble");
    factors.push_back(f);
    check(slod_lod_factor_get_info_member(f, 0, &lod_factor_info), "slod_lod_factor_get_info_member");
    check(slod_lod_factor_inertia(f, 0, &lod_factor_inertia), "slod_lod_factor_inertia");
    return f;
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_heat_irk_ensemble(const int scheme, const unsigned int n_steps, const double dt)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_heat_irk_ensemble: assemble_mass_matrix_ensemble comes first");
    const int          K = (int)par.n_members;
    const std::size_t  ld = (std::size_t)K;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    double *d_u = device_alloc<double>(n_coarse * K);
    double *d_fine = device_alloc<double>(fine_size * K), *d_ell_fine = device_alloc<double>(fine_size * K);
    double *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    ensemble_elliptic_solutions(d_ell_fine);
    slod_lod_factor *f = factor_lod_irk_ensemble(scheme, 1, dt);
    if (hipMemset(d_u, 0, n_coarse * K * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_heat_irk_ensemble: clearing the initial state failed");
    ens_heat_error.assign((std::size_t)n_steps * K, slod_error_norms{});
    source_open(2 * n_steps, (unsigned int)K, true);
    record_open(n_steps, (unsigned int)K, false, true);
    record_state(0, d_u, nullptr);
    for (unsigned int step = 0; step < n_steps; ++step)
      {
        source_arm(2 * step);
        check(slod_lod_irk_heat_steps_ensemble_direct(handle, f, 0, scheme, d_ens_sym, ld, d_ens_cols, dt, 1, K, d_u, ld,
                                                      own_load(d_ens_rhs), ld, 0),
              "slod_lod_irk_heat_steps_ensemble_direct");
        record_state(step + 1, d_u, nullptr);
        check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, d_u, ld, d_fine, fine_size, nullptr),
              "slod_lod_reconstruct_ensemble");
        for (int k = 0; k < K; ++k)
          check(slod_compute_error_norms(handle, (uint32_t)k, d_ell_fine + k * fine_size, d_fine + k * fine_size, nullptr, nullptr,
                                         &ens_heat_error[(std::size_t)step * K + k], nullptr),
                "slod_compute_error_norms");
      }
    record_close();
    drive_open = false;
    ensemble_moment_norms(d_fine, d_mean, d_var, ens_heat_mean_norms, ens_heat_dev_norms);
  }

  template <int dim, int spacedim>
  void LOD<dim, spacedim>::solve_wave_irk_ensemble(const int scheme, const unsigned int n_steps, const double dt)
  {
    if (!d_ens_mass)
      throw std::runtime_error("solve_wave_irk_ensemble: assemble_mass_matrix_ensemble comes first");
    const int          K = (int)par.n_members;
    const std::size_t  ld = (std::size_t)K;
    const unsigned int n_patches = (unsigned int)patches.size();
    const std::size_t  NE = (std::size_t)(1u << par.n_global_refinements) * par.n_subdivisions;
    const std::size_t  fine_size = (NE + 1) * (NE + 1) * spacedim, n_coarse = (std::size_t)n_patches * spacedim;
    double *d_state = device_alloc<double>(2 * n_coarse * K), *d_u = d_state, *d_v = d_u + n_coarse * K;
    double *d_fine = device_alloc<double>(fine_size * K), *d_mean = device_alloc<double>(fine_size), *d_var = device_alloc<double>(fine_size);
    slod_lod_factor *f = factor_lod_irk_ensemble(scheme, 2, dt);
    if (hipMemset(d_state, 0, 2 * n_coarse * K * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      throw std::runtime_error("solve_wave_irk_ensemble: clearing the initial state failed");
    std::vector<double> b(n_coarse * K), u(n_coarse * K);
    if (hipMemcpy(b.data(), d_ens_rhs, b.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("solve_wave_irk_ensemble: download of the loads failed");
    if (load_quiet)
      b.assign(b.size(), 0.0);
    source_open(2 * n_steps, (unsigned int)K, true);
    ens_wave_kinetic.assign((std::size_t)(n_steps + 1) * K, 0.0);
    ens_wave_potential.assign((std::size_t)(n_steps + 1) * K, 0.0);
    ens_wave_work.assign((std::size_t)(n_steps + 1) * K, 0.0);
    std::vector<double> kinetic(2 * ld), potential(2 * ld);
    record_open(n_steps, (unsigned int)K, true, true);
    record_state(0, d_u, d_v);
    for (unsigned int step = 0; step < n_steps; ++step)
      {
        source_arm(2 * step);
        check(slod_lod_irk_wave_steps_ensemble_direct(handle, f, 0, scheme, d_ens_sym, ld, d_ens_mass, ld, d_ens_cols, dt, 0.0, 0.0, 1, K,
                                                      d_u, ld, d_v, ld, own_load(d_ens_rhs), ld, 0, kinetic.data(), potential.data()),
              "slod_lod_irk_wave_steps_ensemble_direct");
        record_state(step + 1, d_u, d_v);
        if (hipMemcpy(u.data(), d_u, u.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
          throw std::runtime_error("solve_wave_irk_ensemble: download of the states failed");
        for (int k = 0; k < K; ++k)
          {
            if (step == 0)
              {
                ens_wave_kinetic[k]   = kinetic[k];
                ens_wave_potential[k] = potential[k];
              }
            ens_wave_kinetic[(std::size_t)(step + 1) * K + k]   = kinetic[ld + k];
            ens_wave_potential[(std::size_t)(step + 1) * K + k] = potential[ld + k];
            double work = 0.0;
            for (std::size_t i = 0; i < n_coarse; ++i)
              work += u[i * K + k] * b[i * K + k];
            ens_wave_work[(std::size_t)(step + 1) * K + k] = work;
          }
      }
    record_close();
    drive_open = false;
    check(slod_lod_reconstruct_ensemble(handle, d_ens_basis, ens_stride, ens_member_stride, K, d_u, ld, d_fine, fine_size, nullptr),
          "slod_lod_reconstruct_ensemble");
    ensemble_moment_norms(d_fine, d_mean, d_var, ens_wave_mean_norms, ens_wave_dev_norms);
  }

  // LOD.cc:1103-1237 with f = 1.  The reference solves with SolverDirect; the CG of the fine problem runs on the
  // coarse grid to the tolerance of the fine solve.
  template <int dim, int spacedim>
  void LOD<dim, spacedim>::assemble_and_solve_coarse_fem_problem()
  {
    if (!d_fem_solution)
      throw std::runtime_error("assemble_and_solve_coarse_fem_problem: assemble_and_solve_fem_problem comes first");
    const std::size_t N = (std::size_t)1 << par.n_global_refinements, NE = N * par.n_subdivisions;
    double           *d_coarse_rhs = device_alloc<double>((N + 1) * (N + 1) * spacedim);
    d_fem_coarse_solution          = device_alloc<double>((N + 1) * (N + 1) * spacedim);
    d_fem_coarse_interpolated      = device_alloc<double>((NE + 1) * (NE + 1) * spacedim);
    check(slod_coarse_fem_rhs(handle, nullptr, d_coarse_rhs, nullptr), "slod_coarse_fem_rhs");
    check(slod_coarse_fem_solve(handle, 0, d_coarse_rhs, d_fem_coarse_solution, fem_rel_tol, fem_max_iterations, nullptr),
          "slod_coarse_fem_solve");
    check(slod_coarse_interpolate(handle, d_fem_coarse_solution, d_fem_coarse_interpolated, nullptr),
          "slod_coarse_interpolate");
    check(slod_compute_error_norms(handle, 0, d_fem_solution, d_fem_coarse_interpolated, nullptr, nullptr, &femH_fem_error,
                                   nullptr),
          "slod_compute_error_norms");
    check(slod_compute_error_norms(handle, 0, d_fem_solution, nullptr, nullptr, nullptr, &fem_norms, nullptr),
          "slod_compute_error_norms");
  }

  template <int dim, int spacedim>
  std::vector<double> LOD<dim, spacedim>::fem_coarse_solution_interpolated() const
  {
    if (!d_fem_coarse_interpolated)
      throw std::runtime_error("fem_coarse_solution_interpolated: assemble_and_solve_coarse_fem_problem comes first");
    const std::size_t   NE = ((std::size_t)1 << par.n_global_refinements) * par.n_subdivisions;
    std::vector<double> v((NE + 1) * (NE + 1) * spacedim);
    // (a blocking copy on the null stream: ordered after the handle's stream, which slod_compute_error_norms left idle)
    if (hipMemcpy(v.data(), d_fem_coarse_interpolated, v.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("fem_coarse_solution_interpolated: download failed");
    return v;
  }

  template class LOD<2, 1>;
  template class LOD<2, 2>;
} // namespace slod
