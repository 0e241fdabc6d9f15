"""The sixteen scripts/bench_*.py scripts at their reduced arguments (18 frames over three sub-batches, windows of 1, 3 and 5
that wrap at both ends; 6 raster frames of 2 distinct sweeps), a time limit for the child process, and the key paths of the
JSON line each printed before the scripts were folded onto scripts/benchlib.py: `a.b` is key b of the dict
under a, `[]` any element of a list.  `library` is the one key the fold added.  bench_submap_search_grid.py runs its fine
stage on window 1 and at one cap beside the fixed one: each of its fine D = 0 calls on the unthinned windows of 3 and 5 sweeps
takes seconds, eighteen of them per window and leaf, and with them the script does not end in five minutes; its coarse stage
keeps the family's windows.  On an MI355X the cases take 2.5 - 21 s, bench_submap_registration.py 72 s and
bench_submap_voxel_registration.py 97 s (the whole tool's ICP is one workgroup per match)."""

_WORLD = ["--frames", "12", "--moved", "6", "--sub-batch", "8"]
_WINDOWS = _WORLD + ["--rounds", "1", "--window-matches", "1:6,3:4,5:2"]
_ONE_STEP = ["--steps", "1", "--warmup", "0"]
_RASTER = ["--frames", "6"] + _ONE_STEP + ["--distinct", "2"]

CASES = {
    "bench_regfront": {"args": ["--frames", "12", "--sub-batch", "8"] + _ONE_STEP + ["--cpu-frames", "1"], "timeout": 60},
    "bench_icp": {"args": ["--frames", "12", "--sub-batch", "8"] + _ONE_STEP + ["--cpu-matches", "1"], "timeout": 60},
    "bench_fine_icp": {"args": _WORLD + _ONE_STEP + ["--cpu-matches", "1"], "timeout": 60},
    "bench_pair_search_grid": {"args": _WORLD + ["--rounds", "1", "--matches", "6"], "timeout": 120},
    "bench_submap_registration": {"args": _WINDOWS, "timeout": 400},
    "bench_submap_voxel_registration": {"args": _WINDOWS, "timeout": 400},
    "bench_submap_coarse_registration": {"args": _WINDOWS, "timeout": 60},
    "bench_submap_pn_voxel_registration": {"args": _WINDOWS, "timeout": 60},
    "bench_submap_top_union": {"args": _WINDOWS, "timeout": 60},
    "bench_submap_search_grid": {"args": _WORLD + ["--rounds", "1", "--window-matches", "1:6", "--coarse-window-matches", "1:6,3:4,5:2",
                                          "--dims", "256"], "timeout": 120},
    "bench_submap_copy_out": {"args": [], "timeout": 60},
    "bench_manip": {"args": _RASTER, "timeout": 60},
    "bench_posed_bev": {"args": _RASTER, "timeout": 60},
    "bench_project": {"args": ["--frames", "6"] + _ONE_STEP + ["--big-frames", "2"], "timeout": 60},
    "bench_submap_bev": {"args": _RASTER + ["--windows", "1,3"], "timeout": 60},
    "bench_submap_float_bev": {"args": _RASTER + ["--windows", "1,3"], "timeout": 60},
}

# the key paths of each parent line, as printed on an MI355X at the arguments above
_KEYS = {
    "bench_regfront": """
checker_single_core_frames_per_s device fenced_frames_per_s fenced_median_ms frames host
kernels_ms_per_step.k_rf_cells kernels_ms_per_step.k_rf_normals kernels_ms_per_step.k_rf_top
kernels_ms_per_step.k_rf_voxel metric records_per_frame_max records_per_frame_mean sensor steps sub_batch
unfenced_frames_per_s unfenced_mean_ms warmup
""",
    "bench_icp": """
checker_single_core_matches_per_s device fenced_matches_per_s fenced_median_ms frames host iterations_mean
kernels_ms_per_step.k_icp kernels_ms_per_step.k_icp_best kernels_ms_per_step.k_icp_grid matches metric problems
records_per_frame_mean sensor states steps unfenced_matches_per_s unfenced_mean_ms warmup
""",
    "bench_fine_icp": """
checker_single_core_matches_per_s device frames host metric runs.bench_icp/top_part.fenced_matches_per_s
runs.bench_icp/top_part.fenced_median_ms runs.bench_icp/top_part.iterations.max
runs.bench_icp/top_part.iterations.mean runs.bench_icp/top_part.iterations.p50 runs.bench_icp/top_part.iterations.p90
runs.bench_icp/top_part.kernels_ms_per_step.k_fine_grid runs.bench_icp/top_part.kernels_ms_per_step.k_fine_icp
runs.bench_icp/top_part.kernels_ms_per_step.k_fine_voxel runs.bench_icp/top_part.matches
runs.bench_icp/top_part.states runs.bench_icp/top_part.success_fitness_le_1_5
runs.bench_icp/top_part.unfenced_matches_per_s runs.bench_icp/top_part.unfenced_mean_ms
runs.bench_icp/whole.fenced_matches_per_s runs.bench_icp/whole.fenced_median_ms runs.bench_icp/whole.iterations.max
runs.bench_icp/whole.iterations.mean runs.bench_icp/whole.iterations.p50 runs.bench_icp/whole.iterations.p90
runs.bench_icp/whole.kernels_ms_per_step.k_fine_grid runs.bench_icp/whole.kernels_ms_per_step.k_fine_icp
runs.bench_icp/whole.kernels_ms_per_step.k_fine_voxel runs.bench_icp/whole.matches runs.bench_icp/whole.states
runs.bench_icp/whole.success_fitness_le_1_5 runs.bench_icp/whole.unfenced_matches_per_s
runs.bench_icp/whole.unfenced_mean_ms runs.moved_copies/top_part.fenced_matches_per_s
runs.moved_copies/top_part.fenced_median_ms runs.moved_copies/top_part.iterations.max
runs.moved_copies/top_part.iterations.mean runs.moved_copies/top_part.iterations.p50
runs.moved_copies/top_part.iterations.p90 runs.moved_copies/top_part.kernels_ms_per_step.k_fine_grid
runs.moved_copies/top_part.kernels_ms_per_step.k_fine_icp runs.moved_copies/top_part.kernels_ms_per_step.k_fine_voxel
runs.moved_copies/top_part.matches runs.moved_copies/top_part.states runs.moved_copies/top_part.success_fitness_le_1_5
runs.moved_copies/top_part.unfenced_matches_per_s runs.moved_copies/top_part.unfenced_mean_ms
runs.moved_copies/whole.fenced_matches_per_s runs.moved_copies/whole.fenced_median_ms
runs.moved_copies/whole.iterations.max runs.moved_copies/whole.iterations.mean runs.moved_copies/whole.iterations.p50
runs.moved_copies/whole.iterations.p90 runs.moved_copies/whole.kernels_ms_per_step.k_fine_grid
runs.moved_copies/whole.kernels_ms_per_step.k_fine_icp runs.moved_copies/whole.kernels_ms_per_step.k_fine_voxel
runs.moved_copies/whole.matches runs.moved_copies/whole.states runs.moved_copies/whole.success_fitness_le_1_5
runs.moved_copies/whole.unfenced_matches_per_s runs.moved_copies/whole.unfenced_mean_ms sensor steps
voxels_per_full_cloud_sample warmup
""",
    "bench_pair_search_grid": """
device equal_pairs every_run_byte_equal_to_its_fixed_grid_partner frames host matches metric rounds runs[].D
runs[].byte_equal runs[].fixed_build_ms runs[].fixed_grid.largest_cell runs[].fixed_grid.max_dim
runs[].fixed_grid.searchable_mean runs[].fixed_grid.targets runs[].fixed_icp_us_per_iteration_problem
runs[].fixed_kernels_ms.k_fine_grid runs[].fixed_kernels_ms.k_fine_icp runs[].fixed_kernels_ms.k_fine_voxel
runs[].fixed_kernels_ms.k_icp runs[].fixed_kernels_ms.k_icp_best runs[].fixed_kernels_ms.k_icp_grid
runs[].fixed_median_ms runs[].fixed_ms runs[].iterations runs[].matches runs[].stage runs[].wide_build_ms
runs[].wide_grid.largest_cell runs[].wide_grid.max_dim runs[].wide_grid.searchable_mean runs[].wide_grid.targets
runs[].wide_icp_us_per_iteration_problem runs[].wide_kernels_ms.k_fine_icp_wide runs[].wide_kernels_ms.k_fine_voxel
runs[].wide_kernels_ms.k_icp_best runs[].wide_kernels_ms.k_icp_wide runs[].wide_kernels_ms.k_pairgrid_desc
runs[].wide_kernels_ms.k_subgrid_bounds runs[].wide_kernels_ms.k_subgrid_count runs[].wide_kernels_ms.k_subgrid_header
runs[].wide_kernels_ms.k_subgrid_scan runs[].wide_kernels_ms.k_subgrid_scatter runs[].wide_kernels_ms.k_subgrid_sums
runs[].wide_median_ms runs[].wide_ms runs[].wide_over_fixed runs[].workload sensor settings.coarse settings.top
settings.whole
""",
    "bench_submap_registration": """
device frames host metric records_per_frame rounds sensor settings windows.1.entries windows.1.identical_to_pair_call
windows.1.k_fine_icp_us_per_iteration_match windows.1.k_submap_icp_us_per_iteration_match windows.1.matches
windows.1.pair_iterations.mean windows.1.pair_iterations.sum windows.1.pair_kernels_ms.k_fine_grid
windows.1.pair_kernels_ms.k_fine_icp windows.1.pair_kernels_ms.k_fine_voxel windows.1.pair_matches_per_s
windows.1.pair_median_ms windows.1.pair_ms windows.1.pair_success_fitness_le_1_5 windows.1.submap_iterations.mean
windows.1.submap_iterations.sum windows.1.submap_kernels_ms.k_fine_voxel windows.1.submap_kernels_ms.k_submap_icp
windows.1.submap_kernels_ms.k_submap_target windows.1.submap_matches_per_s windows.1.submap_median_ms
windows.1.submap_ms windows.1.submap_over_pair windows.1.submap_states windows.1.submap_success_fitness_le_1_5
windows.3.entries windows.3.identical_to_pair_call windows.3.k_fine_icp_us_per_iteration_match
windows.3.k_submap_icp_us_per_iteration_match windows.3.matches windows.3.pair_iterations.mean
windows.3.pair_iterations.sum windows.3.pair_kernels_ms.k_fine_grid windows.3.pair_kernels_ms.k_fine_icp
windows.3.pair_kernels_ms.k_fine_voxel windows.3.pair_matches_per_s windows.3.pair_median_ms windows.3.pair_ms
windows.3.pair_success_fitness_le_1_5 windows.3.submap_iterations.mean windows.3.submap_iterations.sum
windows.3.submap_kernels_ms.k_fine_voxel windows.3.submap_kernels_ms.k_submap_icp
windows.3.submap_kernels_ms.k_submap_target windows.3.submap_matches_per_s windows.3.submap_median_ms
windows.3.submap_ms windows.3.submap_over_pair windows.3.submap_states windows.3.submap_success_fitness_le_1_5
windows.5.entries windows.5.identical_to_pair_call windows.5.k_fine_icp_us_per_iteration_match
windows.5.k_submap_icp_us_per_iteration_match windows.5.matches windows.5.pair_iterations.mean
windows.5.pair_iterations.sum windows.5.pair_kernels_ms.k_fine_grid windows.5.pair_kernels_ms.k_fine_icp
windows.5.pair_kernels_ms.k_fine_voxel windows.5.pair_matches_per_s windows.5.pair_median_ms windows.5.pair_ms
windows.5.pair_success_fitness_le_1_5 windows.5.submap_iterations.mean windows.5.submap_iterations.sum
windows.5.submap_kernels_ms.k_fine_voxel windows.5.submap_kernels_ms.k_submap_icp
windows.5.submap_kernels_ms.k_submap_target windows.5.submap_matches_per_s windows.5.submap_median_ms
windows.5.submap_ms windows.5.submap_over_pair windows.5.submap_states windows.5.submap_success_fitness_le_1_5
""",
    "bench_submap_voxel_registration": """
device frames host map_leaf metric records_per_frame rounds sensor settings windows.1.entries
windows.1.identical_results windows.1.maps_counted windows.1.matches windows.1.matches_whose_verdict_differs
windows.1.plain_icp_us_per_iteration_match windows.1.plain_iterations.mean windows.1.plain_iterations.sum
windows.1.plain_kernels_ms.k_fine_voxel windows.1.plain_kernels_ms.k_submap_icp
windows.1.plain_kernels_ms.k_submap_target windows.1.plain_matches_per_s windows.1.plain_ms.max
windows.1.plain_ms.median windows.1.plain_ms.min windows.1.plain_states windows.1.plain_success_fitness_le_1_5
windows.1.points_per_map_after.max windows.1.points_per_map_after.mean windows.1.points_per_map_after.min
windows.1.points_per_map_before.max windows.1.points_per_map_before.mean windows.1.points_per_map_before.min
windows.1.thin_icp_us_per_iteration_match windows.1.thin_iterations.mean windows.1.thin_iterations.sum
windows.1.thin_kernels_ms.k_fine_voxel windows.1.thin_kernels_ms.k_submap_icp
windows.1.thin_kernels_ms.k_submap_vox_finish windows.1.thin_kernels_ms.k_submap_vox_global
windows.1.thin_kernels_ms.k_submap_vox_keys windows.1.thin_kernels_ms.k_submap_vox_move
windows.1.thin_kernels_ms.k_submap_vox_tile windows.1.thin_matches_per_s windows.1.thin_ms.max
windows.1.thin_ms.median windows.1.thin_ms.min windows.1.thin_over_plain windows.1.thin_stages_ms.centroids_grid
windows.1.thin_stages_ms.icp windows.1.thin_stages_ms.keys windows.1.thin_stages_ms.move windows.1.thin_stages_ms.sort
windows.1.thin_states windows.1.thin_success_fitness_le_1_5 windows.3.entries windows.3.identical_results
windows.3.maps_counted windows.3.matches windows.3.matches_whose_verdict_differs
windows.3.plain_icp_us_per_iteration_match windows.3.plain_iterations.mean windows.3.plain_iterations.sum
windows.3.plain_kernels_ms.k_fine_voxel windows.3.plain_kernels_ms.k_submap_icp
windows.3.plain_kernels_ms.k_submap_target windows.3.plain_matches_per_s windows.3.plain_ms.max
windows.3.plain_ms.median windows.3.plain_ms.min windows.3.plain_states windows.3.plain_success_fitness_le_1_5
windows.3.points_per_map_after.max windows.3.points_per_map_after.mean windows.3.points_per_map_after.min
windows.3.points_per_map_before.max windows.3.points_per_map_before.mean windows.3.points_per_map_before.min
windows.3.thin_icp_us_per_iteration_match windows.3.thin_iterations.mean windows.3.thin_iterations.sum
windows.3.thin_kernels_ms.k_fine_voxel windows.3.thin_kernels_ms.k_submap_icp
windows.3.thin_kernels_ms.k_submap_vox_finish windows.3.thin_kernels_ms.k_submap_vox_global
windows.3.thin_kernels_ms.k_submap_vox_keys windows.3.thin_kernels_ms.k_submap_vox_move
windows.3.thin_kernels_ms.k_submap_vox_tile windows.3.thin_matches_per_s windows.3.thin_ms.max
windows.3.thin_ms.median windows.3.thin_ms.min windows.3.thin_over_plain windows.3.thin_stages_ms.centroids_grid
windows.3.thin_stages_ms.icp windows.3.thin_stages_ms.keys windows.3.thin_stages_ms.move windows.3.thin_stages_ms.sort
windows.3.thin_states windows.3.thin_success_fitness_le_1_5 windows.5.entries windows.5.identical_results
windows.5.maps_counted windows.5.matches windows.5.matches_whose_verdict_differs
windows.5.plain_icp_us_per_iteration_match windows.5.plain_iterations.mean windows.5.plain_iterations.sum
windows.5.plain_kernels_ms.k_fine_voxel windows.5.plain_kernels_ms.k_submap_icp
windows.5.plain_kernels_ms.k_submap_target windows.5.plain_matches_per_s windows.5.plain_ms.max
windows.5.plain_ms.median windows.5.plain_ms.min windows.5.plain_states windows.5.plain_success_fitness_le_1_5
windows.5.points_per_map_after.max windows.5.points_per_map_after.mean windows.5.points_per_map_after.min
windows.5.points_per_map_before.max windows.5.points_per_map_before.mean windows.5.points_per_map_before.min
windows.5.thin_icp_us_per_iteration_match windows.5.thin_iterations.mean windows.5.thin_iterations.sum
windows.5.thin_kernels_ms.k_fine_voxel windows.5.thin_kernels_ms.k_submap_icp
windows.5.thin_kernels_ms.k_submap_vox_finish windows.5.thin_kernels_ms.k_submap_vox_global
windows.5.thin_kernels_ms.k_submap_vox_keys windows.5.thin_kernels_ms.k_submap_vox_move
windows.5.thin_kernels_ms.k_submap_vox_tile windows.5.thin_matches_per_s windows.5.thin_ms.max
windows.5.thin_ms.median windows.5.thin_ms.min windows.5.thin_over_plain windows.5.thin_stages_ms.centroids_grid
windows.5.thin_stages_ms.icp windows.5.thin_stages_ms.keys windows.5.thin_stages_ms.move windows.5.thin_stages_ms.sort
windows.5.thin_states windows.5.thin_success_fitness_le_1_5
""",
    "bench_submap_coarse_registration": """
device frames host metric rounds rows_per_frame.max rows_per_frame.mean sensor settings stride windows.1.entries
windows.1.identical_to_pair_call windows.1.k_icp_us_per_iteration_problem
windows.1.k_submap_coarse_icp_us_per_iteration_problem windows.1.matches windows.1.pair_iterations.mean
windows.1.pair_iterations.sum windows.1.pair_kernels_ms.k_icp windows.1.pair_kernels_ms.k_icp_best
windows.1.pair_kernels_ms.k_icp_grid windows.1.pair_matches_per_s windows.1.pair_median_ms windows.1.pair_ms
windows.1.problems windows.1.submap_best windows.1.submap_iterations.mean windows.1.submap_iterations.sum
windows.1.submap_kernels_ms.k_icp_best windows.1.submap_kernels_ms.k_submap_coarse_icp
windows.1.submap_kernels_ms.k_submap_pn_target windows.1.submap_matches_per_s windows.1.submap_median_ms
windows.1.submap_ms windows.1.submap_over_pair windows.1.submap_states windows.1.target_rows.max
windows.1.target_rows.mean windows.3.entries windows.3.identical_to_pair_call windows.3.k_icp_us_per_iteration_problem
windows.3.k_submap_coarse_icp_us_per_iteration_problem windows.3.matches windows.3.pair_iterations.mean
windows.3.pair_iterations.sum windows.3.pair_kernels_ms.k_icp windows.3.pair_kernels_ms.k_icp_best
windows.3.pair_kernels_ms.k_icp_grid windows.3.pair_matches_per_s windows.3.pair_median_ms windows.3.pair_ms
windows.3.problems windows.3.submap_best windows.3.submap_iterations.mean windows.3.submap_iterations.sum
windows.3.submap_kernels_ms.k_icp_best windows.3.submap_kernels_ms.k_submap_coarse_icp
windows.3.submap_kernels_ms.k_submap_pn_target windows.3.submap_matches_per_s windows.3.submap_median_ms
windows.3.submap_ms windows.3.submap_over_pair windows.3.submap_states windows.3.target_rows.max
windows.3.target_rows.mean windows.5.entries windows.5.identical_to_pair_call windows.5.k_icp_us_per_iteration_problem
windows.5.k_submap_coarse_icp_us_per_iteration_problem windows.5.matches windows.5.pair_iterations.mean
windows.5.pair_iterations.sum windows.5.pair_kernels_ms.k_icp windows.5.pair_kernels_ms.k_icp_best
windows.5.pair_kernels_ms.k_icp_grid windows.5.pair_matches_per_s windows.5.pair_median_ms windows.5.pair_ms
windows.5.problems windows.5.submap_best windows.5.submap_iterations.mean windows.5.submap_iterations.sum
windows.5.submap_kernels_ms.k_icp_best windows.5.submap_kernels_ms.k_submap_coarse_icp
windows.5.submap_kernels_ms.k_submap_pn_target windows.5.submap_matches_per_s windows.5.submap_median_ms
windows.5.submap_ms windows.5.submap_over_pair windows.5.submap_states windows.5.target_rows.max
windows.5.target_rows.mean
""",
    "bench_submap_pn_voxel_registration": """
device frames host metric pn_leaf radius rounds rows_per_frame.max rows_per_frame.mean sensor settings stride
windows.1.best_agree windows.1.entries windows.1.matches windows.1.plain_best windows.1.plain_fitness.above_1.5
windows.1.plain_fitness.max windows.1.plain_fitness.median windows.1.plain_icp_us_per_iteration_problem
windows.1.plain_iterations.mean windows.1.plain_iterations.sum windows.1.plain_kernels_ms.k_icp_best
windows.1.plain_kernels_ms.k_submap_coarse_icp windows.1.plain_kernels_ms.k_submap_pn_target
windows.1.plain_matches_per_s windows.1.plain_median_ms windows.1.plain_ms windows.1.plain_range_ms
windows.1.plain_states windows.1.problems windows.1.rows_after.max windows.1.rows_after.mean windows.1.rows_after.sum
windows.1.rows_before.max windows.1.rows_before.mean windows.1.rows_before.sum windows.1.thinned_best
windows.1.thinned_fitness.above_1.5 windows.1.thinned_fitness.max windows.1.thinned_fitness.median
windows.1.thinned_icp_us_per_iteration_problem windows.1.thinned_iterations.mean windows.1.thinned_iterations.sum
windows.1.thinned_kernels_ms.k_icp_best windows.1.thinned_kernels_ms.k_submap_coarse_icp
windows.1.thinned_kernels_ms.k_submap_pn_finish windows.1.thinned_kernels_ms.k_submap_pn_grid
windows.1.thinned_kernels_ms.k_submap_pn_keys windows.1.thinned_kernels_ms.k_submap_pn_move
windows.1.thinned_kernels_ms.k_submap_pn_normals windows.1.thinned_kernels_ms.k_submap_vox_global
windows.1.thinned_kernels_ms.k_submap_vox_tile windows.1.thinned_matches_per_s windows.1.thinned_median_ms
windows.1.thinned_ms windows.1.thinned_new_stages_ms windows.1.thinned_over_plain windows.1.thinned_range_ms
windows.1.thinned_states windows.3.best_agree windows.3.entries windows.3.matches windows.3.plain_best
windows.3.plain_fitness.above_1.5 windows.3.plain_fitness.max windows.3.plain_fitness.median
windows.3.plain_icp_us_per_iteration_problem windows.3.plain_iterations.mean windows.3.plain_iterations.sum
windows.3.plain_kernels_ms.k_icp_best windows.3.plain_kernels_ms.k_submap_coarse_icp
windows.3.plain_kernels_ms.k_submap_pn_target windows.3.plain_matches_per_s windows.3.plain_median_ms
windows.3.plain_ms windows.3.plain_range_ms windows.3.plain_states windows.3.problems windows.3.rows_after.max
windows.3.rows_after.mean windows.3.rows_after.sum windows.3.rows_before.max windows.3.rows_before.mean
windows.3.rows_before.sum windows.3.thinned_best windows.3.thinned_fitness.above_1.5 windows.3.thinned_fitness.max
windows.3.thinned_fitness.median windows.3.thinned_icp_us_per_iteration_problem windows.3.thinned_iterations.mean
windows.3.thinned_iterations.sum windows.3.thinned_kernels_ms.k_icp_best
windows.3.thinned_kernels_ms.k_submap_coarse_icp windows.3.thinned_kernels_ms.k_submap_pn_finish
windows.3.thinned_kernels_ms.k_submap_pn_grid windows.3.thinned_kernels_ms.k_submap_pn_keys
windows.3.thinned_kernels_ms.k_submap_pn_move windows.3.thinned_kernels_ms.k_submap_pn_normals
windows.3.thinned_kernels_ms.k_submap_vox_global windows.3.thinned_kernels_ms.k_submap_vox_tile
windows.3.thinned_matches_per_s windows.3.thinned_median_ms windows.3.thinned_ms windows.3.thinned_new_stages_ms
windows.3.thinned_over_plain windows.3.thinned_range_ms windows.3.thinned_states windows.5.best_agree
windows.5.entries windows.5.matches windows.5.plain_best windows.5.plain_fitness.above_1.5 windows.5.plain_fitness.max
windows.5.plain_fitness.median windows.5.plain_icp_us_per_iteration_problem windows.5.plain_iterations.mean
windows.5.plain_iterations.sum windows.5.plain_kernels_ms.k_icp_best windows.5.plain_kernels_ms.k_submap_coarse_icp
windows.5.plain_kernels_ms.k_submap_pn_target windows.5.plain_matches_per_s windows.5.plain_median_ms
windows.5.plain_ms windows.5.plain_range_ms windows.5.plain_states windows.5.problems windows.5.rows_after.max
windows.5.rows_after.mean windows.5.rows_after.sum windows.5.rows_before.max windows.5.rows_before.mean
windows.5.rows_before.sum windows.5.thinned_best windows.5.thinned_fitness.above_1.5 windows.5.thinned_fitness.max
windows.5.thinned_fitness.median windows.5.thinned_icp_us_per_iteration_problem windows.5.thinned_iterations.mean
windows.5.thinned_iterations.sum windows.5.thinned_kernels_ms.k_icp_best
windows.5.thinned_kernels_ms.k_submap_coarse_icp windows.5.thinned_kernels_ms.k_submap_pn_finish
windows.5.thinned_kernels_ms.k_submap_pn_grid windows.5.thinned_kernels_ms.k_submap_pn_keys
windows.5.thinned_kernels_ms.k_submap_pn_move windows.5.thinned_kernels_ms.k_submap_pn_normals
windows.5.thinned_kernels_ms.k_submap_vox_global windows.5.thinned_kernels_ms.k_submap_vox_tile
windows.5.thinned_matches_per_s windows.5.thinned_median_ms windows.5.thinned_ms windows.5.thinned_new_stages_ms
windows.5.thinned_over_plain windows.5.thinned_range_ms windows.5.thinned_states
""",
    "bench_submap_top_union": """
device frames front_end_kernels_ms_of_all_frames.k_rf_cells front_end_kernels_ms_of_all_frames.k_rf_normals
front_end_kernels_ms_of_all_frames.k_rf_top front_end_kernels_ms_of_all_frames.k_rf_voxel
front_end_ms_per_frame_in_a_batch host labelled_records_of_frame_0 metric pn_leaf radius records_per_frame rounds
rows_per_frame.max rows_per_frame.mean sensor settings stride windows.1.best_agree windows.1.concatenation_best
windows.1.concatenation_fitness.above_1.5 windows.1.concatenation_fitness.max windows.1.concatenation_fitness.median
windows.1.concatenation_icp_us_per_iteration_problem windows.1.concatenation_iterations.mean
windows.1.concatenation_iterations.sum windows.1.concatenation_kernels_ms.k_icp_best
windows.1.concatenation_kernels_ms.k_submap_coarse_icp windows.1.concatenation_kernels_ms.k_submap_pn_finish
windows.1.concatenation_kernels_ms.k_submap_pn_grid windows.1.concatenation_kernels_ms.k_submap_pn_keys
windows.1.concatenation_kernels_ms.k_submap_pn_move windows.1.concatenation_kernels_ms.k_submap_pn_normals
windows.1.concatenation_kernels_ms.k_submap_vox_global windows.1.concatenation_kernels_ms.k_submap_vox_tile
windows.1.concatenation_matches_per_s windows.1.concatenation_median_ms windows.1.concatenation_ms
windows.1.concatenation_range_ms windows.1.concatenation_states windows.1.entries windows.1.frames_named
windows.1.front_end_ms_of_named_frames windows.1.front_end_ms_per_frame_of_one_window_alone
windows.1.front_end_top_stage_kernels_ms.k_rf_cells windows.1.front_end_top_stage_kernels_ms.k_rf_normals
windows.1.front_end_top_stage_kernels_ms.k_rf_top windows.1.front_end_top_stage_kernels_ms.k_rf_voxel
windows.1.front_end_top_stage_ms_of_w_frames_at_batch_throughput windows.1.front_end_top_stage_ms_per_window_of_sweeps
windows.1.front_end_top_stage_ms_rounds windows.1.matches windows.1.problems windows.1.rows_concatenation.max
windows.1.rows_concatenation.mean windows.1.rows_concatenation.sum windows.1.rows_top_before_thinning.max
windows.1.rows_top_before_thinning.mean windows.1.rows_union.max windows.1.rows_union.mean windows.1.rows_union.sum
windows.1.selection_kernels_ms.k_submap_pn_out windows.1.selection_kernels_ms.k_submap_top_cells
windows.1.selection_kernels_ms.k_submap_top_compact windows.1.selection_kernels_ms.k_submap_top_hist
windows.1.selection_kernels_ms.k_submap_top_keys windows.1.selection_kernels_ms.k_submap_top_rows
windows.1.selection_kernels_ms.k_submap_top_scan windows.1.selection_kernels_ms.k_submap_vox_global
windows.1.selection_kernels_ms.k_submap_vox_tile windows.1.selection_ms_per_map windows.1.selection_ms_rounds
windows.1.selection_over_front_end_top_stage windows.1.selection_over_front_end_top_stage_at_batch_throughput
windows.1.union_best windows.1.union_fitness.above_1.5 windows.1.union_fitness.max windows.1.union_fitness.median
windows.1.union_icp_us_per_iteration_problem windows.1.union_iterations.mean windows.1.union_iterations.sum
windows.1.union_kernels_ms.k_icp_best windows.1.union_kernels_ms.k_submap_coarse_icp
windows.1.union_kernels_ms.k_submap_pn_finish windows.1.union_kernels_ms.k_submap_pn_grid
windows.1.union_kernels_ms.k_submap_pn_keys windows.1.union_kernels_ms.k_submap_pn_normals
windows.1.union_kernels_ms.k_submap_top_cells windows.1.union_kernels_ms.k_submap_top_compact
windows.1.union_kernels_ms.k_submap_top_hist windows.1.union_kernels_ms.k_submap_top_keys
windows.1.union_kernels_ms.k_submap_top_overflow windows.1.union_kernels_ms.k_submap_top_rows
windows.1.union_kernels_ms.k_submap_top_scan windows.1.union_kernels_ms.k_submap_vox_global
windows.1.union_kernels_ms.k_submap_vox_tile windows.1.union_matches_per_s windows.1.union_median_ms
windows.1.union_ms windows.1.union_new_kernels_ms windows.1.union_new_kernels_share windows.1.union_over_concatenation
windows.1.union_range_ms windows.1.union_records_per_map windows.1.union_states windows.3.best_agree
windows.3.concatenation_best windows.3.concatenation_fitness.above_1.5 windows.3.concatenation_fitness.max
windows.3.concatenation_fitness.median windows.3.concatenation_icp_us_per_iteration_problem
windows.3.concatenation_iterations.mean windows.3.concatenation_iterations.sum
windows.3.concatenation_kernels_ms.k_icp_best windows.3.concatenation_kernels_ms.k_submap_coarse_icp
windows.3.concatenation_kernels_ms.k_submap_pn_finish windows.3.concatenation_kernels_ms.k_submap_pn_grid
windows.3.concatenation_kernels_ms.k_submap_pn_keys windows.3.concatenation_kernels_ms.k_submap_pn_move
windows.3.concatenation_kernels_ms.k_submap_pn_normals windows.3.concatenation_kernels_ms.k_submap_vox_global
windows.3.concatenation_kernels_ms.k_submap_vox_tile windows.3.concatenation_matches_per_s
windows.3.concatenation_median_ms windows.3.concatenation_ms windows.3.concatenation_range_ms
windows.3.concatenation_states windows.3.entries windows.3.frames_named windows.3.front_end_ms_of_named_frames
windows.3.front_end_ms_per_frame_of_one_window_alone windows.3.front_end_top_stage_kernels_ms.k_rf_cells
windows.3.front_end_top_stage_kernels_ms.k_rf_normals windows.3.front_end_top_stage_kernels_ms.k_rf_top
windows.3.front_end_top_stage_kernels_ms.k_rf_voxel windows.3.front_end_top_stage_ms_of_w_frames_at_batch_throughput
windows.3.front_end_top_stage_ms_per_window_of_sweeps windows.3.front_end_top_stage_ms_rounds windows.3.matches
windows.3.problems windows.3.rows_concatenation.max windows.3.rows_concatenation.mean windows.3.rows_concatenation.sum
windows.3.rows_top_before_thinning.max windows.3.rows_top_before_thinning.mean windows.3.rows_union.max
windows.3.rows_union.mean windows.3.rows_union.sum windows.3.selection_kernels_ms.k_submap_pn_out
windows.3.selection_kernels_ms.k_submap_top_cells windows.3.selection_kernels_ms.k_submap_top_compact
windows.3.selection_kernels_ms.k_submap_top_hist windows.3.selection_kernels_ms.k_submap_top_keys
windows.3.selection_kernels_ms.k_submap_top_rows windows.3.selection_kernels_ms.k_submap_top_scan
windows.3.selection_kernels_ms.k_submap_vox_global windows.3.selection_kernels_ms.k_submap_vox_tile
windows.3.selection_ms_per_map windows.3.selection_ms_rounds windows.3.selection_over_front_end_top_stage
windows.3.selection_over_front_end_top_stage_at_batch_throughput windows.3.union_best
windows.3.union_fitness.above_1.5 windows.3.union_fitness.max windows.3.union_fitness.median
windows.3.union_icp_us_per_iteration_problem windows.3.union_iterations.mean windows.3.union_iterations.sum
windows.3.union_kernels_ms.k_icp_best windows.3.union_kernels_ms.k_submap_coarse_icp
windows.3.union_kernels_ms.k_submap_pn_finish windows.3.union_kernels_ms.k_submap_pn_grid
windows.3.union_kernels_ms.k_submap_pn_keys windows.3.union_kernels_ms.k_submap_pn_normals
windows.3.union_kernels_ms.k_submap_top_cells windows.3.union_kernels_ms.k_submap_top_compact
windows.3.union_kernels_ms.k_submap_top_hist windows.3.union_kernels_ms.k_submap_top_keys
windows.3.union_kernels_ms.k_submap_top_overflow windows.3.union_kernels_ms.k_submap_top_rows
windows.3.union_kernels_ms.k_submap_top_scan windows.3.union_kernels_ms.k_submap_vox_global
windows.3.union_kernels_ms.k_submap_vox_tile windows.3.union_matches_per_s windows.3.union_median_ms
windows.3.union_ms windows.3.union_new_kernels_ms windows.3.union_new_kernels_share windows.3.union_over_concatenation
windows.3.union_range_ms windows.3.union_records_per_map windows.3.union_states windows.5.best_agree
windows.5.concatenation_best windows.5.concatenation_fitness.above_1.5 windows.5.concatenation_fitness.max
windows.5.concatenation_fitness.median windows.5.concatenation_icp_us_per_iteration_problem
windows.5.concatenation_iterations.mean windows.5.concatenation_iterations.sum
windows.5.concatenation_kernels_ms.k_icp_best windows.5.concatenation_kernels_ms.k_submap_coarse_icp
windows.5.concatenation_kernels_ms.k_submap_pn_finish windows.5.concatenation_kernels_ms.k_submap_pn_grid
windows.5.concatenation_kernels_ms.k_submap_pn_keys windows.5.concatenation_kernels_ms.k_submap_pn_move
windows.5.concatenation_kernels_ms.k_submap_pn_normals windows.5.concatenation_kernels_ms.k_submap_vox_global
windows.5.concatenation_kernels_ms.k_submap_vox_tile windows.5.concatenation_matches_per_s
windows.5.concatenation_median_ms windows.5.concatenation_ms windows.5.concatenation_range_ms
windows.5.concatenation_states windows.5.entries windows.5.frames_named windows.5.front_end_ms_of_named_frames
windows.5.front_end_ms_per_frame_of_one_window_alone windows.5.front_end_top_stage_kernels_ms.k_rf_cells
windows.5.front_end_top_stage_kernels_ms.k_rf_normals windows.5.front_end_top_stage_kernels_ms.k_rf_top
windows.5.front_end_top_stage_kernels_ms.k_rf_voxel windows.5.front_end_top_stage_ms_of_w_frames_at_batch_throughput
windows.5.front_end_top_stage_ms_per_window_of_sweeps windows.5.front_end_top_stage_ms_rounds windows.5.matches
windows.5.problems windows.5.rows_concatenation.max windows.5.rows_concatenation.mean windows.5.rows_concatenation.sum
windows.5.rows_top_before_thinning.max windows.5.rows_top_before_thinning.mean windows.5.rows_union.max
windows.5.rows_union.mean windows.5.rows_union.sum windows.5.selection_kernels_ms.k_submap_pn_out
windows.5.selection_kernels_ms.k_submap_top_cells windows.5.selection_kernels_ms.k_submap_top_compact
windows.5.selection_kernels_ms.k_submap_top_hist windows.5.selection_kernels_ms.k_submap_top_keys
windows.5.selection_kernels_ms.k_submap_top_rows windows.5.selection_kernels_ms.k_submap_top_scan
windows.5.selection_kernels_ms.k_submap_vox_global windows.5.selection_kernels_ms.k_submap_vox_tile
windows.5.selection_ms_per_map windows.5.selection_ms_rounds windows.5.selection_over_front_end_top_stage
windows.5.selection_over_front_end_top_stage_at_batch_throughput windows.5.union_best
windows.5.union_fitness.above_1.5 windows.5.union_fitness.max windows.5.union_fitness.median
windows.5.union_icp_us_per_iteration_problem windows.5.union_iterations.mean windows.5.union_iterations.sum
windows.5.union_kernels_ms.k_icp_best windows.5.union_kernels_ms.k_submap_coarse_icp
windows.5.union_kernels_ms.k_submap_pn_finish windows.5.union_kernels_ms.k_submap_pn_grid
windows.5.union_kernels_ms.k_submap_pn_keys windows.5.union_kernels_ms.k_submap_pn_normals
windows.5.union_kernels_ms.k_submap_top_cells windows.5.union_kernels_ms.k_submap_top_compact
windows.5.union_kernels_ms.k_submap_top_hist windows.5.union_kernels_ms.k_submap_top_keys
windows.5.union_kernels_ms.k_submap_top_overflow windows.5.union_kernels_ms.k_submap_top_rows
windows.5.union_kernels_ms.k_submap_top_scan windows.5.union_kernels_ms.k_submap_vox_global
windows.5.union_kernels_ms.k_submap_vox_tile windows.5.union_matches_per_s windows.5.union_median_ms
windows.5.union_ms windows.5.union_new_kernels_ms windows.5.union_new_kernels_share windows.5.union_over_concatenation
windows.5.union_range_ms windows.5.union_records_per_map windows.5.union_states
""",
    "bench_submap_search_grid": """
device every_run_byte_equal_to_its_fixed_grid_partner frames host map_leaf metric pn_leaf rounds runs[].D
runs[].byte_equal runs[].fixed_build_kernels_ms runs[].fixed_grid.largest_cell runs[].fixed_grid.maps
runs[].fixed_grid.max_dim runs[].fixed_grid.searchable_mean runs[].fixed_icp_us_per_iteration_problem
runs[].fixed_kernels_ms.k_submap_coarse_icp runs[].fixed_kernels_ms.k_submap_icp
runs[].fixed_kernels_ms.k_submap_pn_finish runs[].fixed_kernels_ms.k_submap_pn_grid
runs[].fixed_kernels_ms.k_submap_pn_keys runs[].fixed_kernels_ms.k_submap_pn_move
runs[].fixed_kernels_ms.k_submap_pn_normals runs[].fixed_kernels_ms.k_submap_pn_target
runs[].fixed_kernels_ms.k_submap_target runs[].fixed_kernels_ms.k_submap_vox_finish
runs[].fixed_kernels_ms.k_submap_vox_global runs[].fixed_kernels_ms.k_submap_vox_keys
runs[].fixed_kernels_ms.k_submap_vox_move runs[].fixed_kernels_ms.k_submap_vox_tile runs[].fixed_median_ms
runs[].fixed_ms runs[].iterations runs[].leaf runs[].matches runs[].stage runs[].wide_build_ms
runs[].wide_grid.largest_cell runs[].wide_grid.maps runs[].wide_grid.max_dim runs[].wide_grid.searchable_mean
runs[].wide_icp_us_per_iteration_problem runs[].wide_kernels_ms.k_subgrid_bounds
runs[].wide_kernels_ms.k_subgrid_count runs[].wide_kernels_ms.k_subgrid_header runs[].wide_kernels_ms.k_subgrid_scan
runs[].wide_kernels_ms.k_subgrid_scatter runs[].wide_kernels_ms.k_subgrid_sums
runs[].wide_kernels_ms.k_submap_coarse_icp_wide runs[].wide_kernels_ms.k_submap_icp_wide
runs[].wide_kernels_ms.k_submap_pn_finish runs[].wide_kernels_ms.k_submap_pn_keys
runs[].wide_kernels_ms.k_submap_pn_move runs[].wide_kernels_ms.k_submap_pn_normals
runs[].wide_kernels_ms.k_submap_vox_finish runs[].wide_kernels_ms.k_submap_vox_global
runs[].wide_kernels_ms.k_submap_vox_keys runs[].wide_kernels_ms.k_submap_vox_move
runs[].wide_kernels_ms.k_submap_vox_tile runs[].wide_median_ms runs[].wide_ms runs[].wide_over_fixed runs[].window
sensor settings.coarse settings.fine
""",
    "bench_submap_copy_out": """
pn.kernel pn.ms_per_launch_by_batch pn.rows_copied_per_launch vox.kernel vox.ms_per_launch_by_batch
vox.rows_copied_per_launch
""",
    "bench_manip": """
device frames host interval library metric n_poses.0.achieved_GBps_over_kernel_time
n_poses.0.algorithmic_bytes_per_frame n_poses.0.fenced_frames_per_s n_poses.0.fenced_median_ms
n_poses.0.kernel_ms_per_step n_poses.0.unfenced_frames_per_s n_poses.0.unfenced_mean_ms
n_poses.1.achieved_GBps_over_kernel_time n_poses.1.algorithmic_bytes_per_frame n_poses.1.fenced_frames_per_s
n_poses.1.fenced_median_ms n_poses.1.kernel_ms_per_step n_poses.1.unfenced_frames_per_s n_poses.1.unfenced_mean_ms
n_poses.8.achieved_GBps_over_kernel_time n_poses.8.algorithmic_bytes_per_frame n_poses.8.fenced_frames_per_s
n_poses.8.fenced_median_ms n_poses.8.kernel_ms_per_step n_poses.8.unfenced_frames_per_s n_poses.8.unfenced_mean_ms
records_per_frame skip_label0 steps warmup
""",
    "bench_posed_bev": """
batch_over_per_cloud_at_1_pose batch_over_per_cloud_at_8_poses device frames host layers library mat_size metric
n_poses.0.algorithmic_bytes_per_grid n_poses.0.expand_us_per_grid n_poses.0.expand_written_GBps
n_poses.0.fenced_grids_per_s n_poses.0.fenced_median_ms n_poses.0.float_bev_yardstick.fenced_grids_per_s
n_poses.0.float_bev_yardstick.fenced_median_ms n_poses.0.float_bev_yardstick.kernel_us_per_grid
n_poses.0.float_bev_yardstick.kernels.k_float_bev_batch.launches
n_poses.0.float_bev_yardstick.kernels.k_float_bev_batch.ms_per_step n_poses.0.float_bev_yardstick.unfenced_grids_per_s
n_poses.0.float_bev_yardstick.unfenced_mean_ms n_poses.0.grids n_poses.0.kernels.k_posed_expand.launches
n_poses.0.kernels.k_posed_expand.ms_per_step n_poses.0.kernels.k_posed_splat.launches
n_poses.0.kernels.k_posed_splat.ms_per_step n_poses.0.posed_over_float_unfenced_time n_poses.0.splat_over_float_kernel
n_poses.0.splat_us_per_grid n_poses.0.unfenced_grids_per_s n_poses.0.unfenced_mean_ms
n_poses.1.algorithmic_bytes_per_grid n_poses.1.expand_us_per_grid n_poses.1.expand_written_GBps
n_poses.1.fenced_grids_per_s n_poses.1.fenced_median_ms n_poses.1.float_bev_yardstick.fenced_grids_per_s
n_poses.1.float_bev_yardstick.fenced_median_ms n_poses.1.float_bev_yardstick.kernel_us_per_grid
n_poses.1.float_bev_yardstick.kernels.k_float_bev_batch.launches
n_poses.1.float_bev_yardstick.kernels.k_float_bev_batch.ms_per_step n_poses.1.float_bev_yardstick.unfenced_grids_per_s
n_poses.1.float_bev_yardstick.unfenced_mean_ms n_poses.1.grids n_poses.1.kernels.k_posed_expand.launches
n_poses.1.kernels.k_posed_expand.ms_per_step n_poses.1.kernels.k_posed_splat.launches
n_poses.1.kernels.k_posed_splat.ms_per_step n_poses.1.posed_over_float_unfenced_time n_poses.1.splat_over_float_kernel
n_poses.1.splat_us_per_grid n_poses.1.unfenced_grids_per_s n_poses.1.unfenced_mean_ms
n_poses.8.algorithmic_bytes_per_grid n_poses.8.expand_us_per_grid n_poses.8.expand_written_GBps
n_poses.8.fenced_grids_per_s n_poses.8.fenced_median_ms n_poses.8.float_bev_yardstick.fenced_grids_per_s
n_poses.8.float_bev_yardstick.fenced_median_ms n_poses.8.float_bev_yardstick.kernel_us_per_grid
n_poses.8.float_bev_yardstick.kernels.k_float_bev_batch.launches
n_poses.8.float_bev_yardstick.kernels.k_float_bev_batch.ms_per_step n_poses.8.float_bev_yardstick.unfenced_grids_per_s
n_poses.8.float_bev_yardstick.unfenced_mean_ms n_poses.8.grids n_poses.8.kernels.k_posed_expand.launches
n_poses.8.kernels.k_posed_expand.ms_per_step n_poses.8.kernels.k_posed_splat.launches
n_poses.8.kernels.k_posed_splat.ms_per_step n_poses.8.posed_over_float_unfenced_time n_poses.8.splat_over_float_kernel
n_poses.8.splat_us_per_grid n_poses.8.unfenced_grids_per_s n_poses.8.unfenced_mean_ms outputs
per_cloud_transform_multi_single_loop.grids_per_s per_cloud_transform_multi_single_loop.passes_ms posed_group_env
records_per_frame steps warmup
""",
    "bench_project": """
device frames host metric mulran_end_to_end.frame_modes_of_the_last_sub_batch
mulran_end_to_end.passes[].process_alone_fenced_frames_per_s
mulran_end_to_end.passes[].process_alone_unfenced_frames_per_s
mulran_end_to_end.passes[].project_and_process_fenced_frames_per_s
mulran_end_to_end.passes[].project_and_process_unfenced_frames_per_s steps warmup
workloads.kitti_120k.achieved_GBps_over_kernel_time workloads.kitti_120k.algorithmic_bytes_per_frame
workloads.kitti_120k.fenced_frames_per_s workloads.kitti_120k.fenced_median_ms workloads.kitti_120k.frames
workloads.kitti_120k.kernels_ms_per_step.k_kitti_assign workloads.kitti_120k.kernels_ms_per_step.k_kitti_chain
workloads.kitti_120k.kernels_ms_per_step.k_kitti_crossings workloads.kitti_120k.kernels_ms_per_step.k_kitti_gather
workloads.kitti_120k.kind workloads.kitti_120k.returns_per_frame_mean workloads.kitti_120k.sensor
workloads.kitti_120k.unfenced_frames_per_s workloads.kitti_120k.unfenced_mean_ms
workloads.mulran_65536.achieved_GBps_over_kernel_time workloads.mulran_65536.algorithmic_bytes_per_frame
workloads.mulran_65536.fenced_frames_per_s workloads.mulran_65536.fenced_median_ms workloads.mulran_65536.frames
workloads.mulran_65536.kernels_ms_per_step.k_project workloads.mulran_65536.kind
workloads.mulran_65536.returns_per_frame_mean workloads.mulran_65536.sensor
workloads.mulran_65536.unfenced_frames_per_s workloads.mulran_65536.unfenced_mean_ms
workloads.oxford_2M.achieved_GBps_over_kernel_time workloads.oxford_2M.algorithmic_bytes_per_frame
workloads.oxford_2M.fenced_frames_per_s workloads.oxford_2M.fenced_median_ms workloads.oxford_2M.frames
workloads.oxford_2M.kernels_ms_per_step.k_project workloads.oxford_2M.kind workloads.oxford_2M.returns_per_frame_mean
workloads.oxford_2M.sensor workloads.oxford_2M.unfenced_frames_per_s workloads.oxford_2M.unfenced_mean_ms
workloads.oxford_35k.achieved_GBps_over_kernel_time workloads.oxford_35k.algorithmic_bytes_per_frame
workloads.oxford_35k.fenced_frames_per_s workloads.oxford_35k.fenced_median_ms workloads.oxford_35k.frames
workloads.oxford_35k.kernels_ms_per_step.k_project workloads.oxford_35k.kind
workloads.oxford_35k.returns_per_frame_mean workloads.oxford_35k.sensor workloads.oxford_35k.unfenced_frames_per_s
workloads.oxford_35k.unfenced_mean_ms
""",
    "bench_submap_bev": """
device frames host layers library mat_size metric outputs posed_group_env records_per_frame runs steps warmup
windows.1.entries windows.1.half_window windows.1.kernels.k_posed_expand.launches
windows.1.kernels.k_posed_expand.ms_per_step windows.1.kernels.k_submap_splat.launches
windows.1.kernels.k_submap_splat.ms_of_5_steps windows.1.kernels.k_submap_splat.ms_per_step windows.1.launch_groups
windows.1.maps windows.1.maps_per_s windows.1.one_entry_per_map.k_submap_splat_ms_of_5_steps
windows.1.one_entry_per_map.launch_groups windows.1.one_entry_per_map.maps windows.1.point_poses
windows.1.point_poses_per_s windows.1.posed_yardstick.grids windows.1.posed_yardstick.kernels.k_posed_expand.launches
windows.1.posed_yardstick.kernels.k_posed_expand.ms_per_step windows.1.posed_yardstick.kernels.k_posed_splat.launches
windows.1.posed_yardstick.kernels.k_posed_splat.ms_of_5_steps
windows.1.posed_yardstick.kernels.k_posed_splat.ms_per_step windows.1.posed_yardstick.launch_groups
windows.1.posed_yardstick.point_poses windows.1.posed_yardstick.point_poses_per_s
windows.1.posed_yardstick.splat_ns_per_kilo_point_pose windows.1.runs.posed[].fenced_median_ms
windows.1.runs.posed[].unfenced_mean_ms windows.1.runs.submap[].fenced_median_ms
windows.1.runs.submap[].unfenced_mean_ms windows.1.splat_ns_per_kilo_point_pose
windows.1.submap_over_posed_fenced_time windows.1.submap_over_posed_splat_per_point_pose
windows.1.submap_over_posed_unfenced_time windows.3.entries windows.3.half_window
windows.3.kernels.k_posed_expand.launches windows.3.kernels.k_posed_expand.ms_per_step
windows.3.kernels.k_submap_splat.launches windows.3.kernels.k_submap_splat.ms_of_5_steps
windows.3.kernels.k_submap_splat.ms_per_step windows.3.launch_groups windows.3.maps windows.3.maps_per_s
windows.3.one_entry_per_map.k_submap_splat_ms_of_5_steps windows.3.one_entry_per_map.launch_groups
windows.3.one_entry_per_map.maps windows.3.point_poses windows.3.point_poses_per_s windows.3.posed_yardstick.grids
windows.3.posed_yardstick.kernels.k_posed_expand.launches windows.3.posed_yardstick.kernels.k_posed_expand.ms_per_step
windows.3.posed_yardstick.kernels.k_posed_splat.launches windows.3.posed_yardstick.kernels.k_posed_splat.ms_of_5_steps
windows.3.posed_yardstick.kernels.k_posed_splat.ms_per_step windows.3.posed_yardstick.launch_groups
windows.3.posed_yardstick.point_poses windows.3.posed_yardstick.point_poses_per_s
windows.3.posed_yardstick.splat_ns_per_kilo_point_pose windows.3.runs.posed[].fenced_median_ms
windows.3.runs.posed[].unfenced_mean_ms windows.3.runs.submap[].fenced_median_ms
windows.3.runs.submap[].unfenced_mean_ms windows.3.splat_ns_per_kilo_point_pose
windows.3.submap_over_posed_fenced_time windows.3.submap_over_posed_splat_per_point_pose
windows.3.submap_over_posed_unfenced_time
""",
    "bench_submap_float_bev": """
device frames interval library mat_size metric records_per_frame runs skip_label0 steps warmup windows.1.entries
windows.1.float_yardstick.frames_per_s windows.1.float_yardstick.grids
windows.1.float_yardstick.kernels.k_float_bev_batch.launches
windows.1.float_yardstick.kernels.k_float_bev_batch.ms_of_5_steps
windows.1.float_yardstick.kernels.k_float_bev_batch.ms_per_step windows.1.float_yardstick.point_poses
windows.1.float_yardstick.point_poses_per_s windows.1.float_yardstick.splat_ns_per_kilo_point_pose
windows.1.half_window windows.1.kernels.k_submap_float_splat.launches
windows.1.kernels.k_submap_float_splat.ms_of_5_steps windows.1.kernels.k_submap_float_splat.ms_per_step windows.1.maps
windows.1.maps_per_s windows.1.one_entry_per_map.k_submap_float_splat_ms_of_5_steps windows.1.one_entry_per_map.maps
windows.1.one_entry_per_map.splat_ns_per_kilo_point_pose windows.1.oracle_checked_map windows.1.point_poses
windows.1.point_poses_per_s windows.1.runs.float[].fenced_median_ms windows.1.runs.float[].unfenced_mean_ms
windows.1.runs.submap[].fenced_median_ms windows.1.runs.submap[].unfenced_mean_ms
windows.1.splat_ns_per_kilo_point_pose windows.1.submap_over_float_fenced_time
windows.1.submap_over_float_splat_per_point_pose windows.1.submap_over_float_unfenced_time windows.3.entries
windows.3.float_yardstick.frames_per_s windows.3.float_yardstick.grids
windows.3.float_yardstick.kernels.k_float_bev_batch.launches
windows.3.float_yardstick.kernels.k_float_bev_batch.ms_of_5_steps
windows.3.float_yardstick.kernels.k_float_bev_batch.ms_per_step windows.3.float_yardstick.point_poses
windows.3.float_yardstick.point_poses_per_s windows.3.float_yardstick.splat_ns_per_kilo_point_pose
windows.3.half_window windows.3.kernels.k_submap_float_splat.launches
windows.3.kernels.k_submap_float_splat.ms_of_5_steps windows.3.kernels.k_submap_float_splat.ms_per_step windows.3.maps
windows.3.maps_per_s windows.3.one_entry_per_map.k_submap_float_splat_ms_of_5_steps windows.3.one_entry_per_map.maps
windows.3.one_entry_per_map.splat_ns_per_kilo_point_pose windows.3.oracle_checked_map windows.3.point_poses
windows.3.point_poses_per_s windows.3.runs.float[].fenced_median_ms windows.3.runs.float[].unfenced_mean_ms
windows.3.runs.submap[].fenced_median_ms windows.3.runs.submap[].unfenced_mean_ms
windows.3.splat_ns_per_kilo_point_pose windows.3.submap_over_float_fenced_time
windows.3.submap_over_float_splat_per_point_pose windows.3.submap_over_float_unfenced_time
""",
}
for _name, _case in CASES.items():
    _case["keys"] = _KEYS[_name].split()
