"""Loader for ``libmegastep_hip.so`` - the hipcc-built gfx950 library behind ``include/megastep_hip.h``.

Counterpart of the reference's JIT build-and-load at import (reference: megastep/__init__.py:7-20): the library is
built in-tree with hipcc (``csrc/Makefile``) and bound with ctypes. There is NO fallback: if the library cannot be
built or loaded, or no HIP device is visible when a kernel is requested, this raises.
"""
import ctypes as C
import os
import subprocess
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
# MEGASTEP_HIP_LIB points at an alternative build of the same ABI (A/B experiments); default is the in-tree build
LIB_PATH = os.environ.get('MEGASTEP_HIP_LIB') or os.path.join(CSRC, 'libmegastep_hip.so')
ABI_VERSION = 17

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int)


class MsConfig(C.Structure):
    _fields_ = [('agent_radius', C.c_float), ('res', C.c_int), ('fov', C.c_float), ('fps', C.c_float)]


class MsScenery(C.Structure):
    _fields_ = [
        ('n_envs', C.c_int), ('n_agents', C.c_int), ('n_model', C.c_int),
        ('lights_vals', C.c_void_p), ('lights_widths', C.c_void_p), ('lights_starts', C.c_void_p),
        ('lines_vals', C.c_void_p), ('lines_widths', C.c_void_p), ('lines_starts', C.c_void_p),
        ('lines_inverse', C.c_void_p),
        ('textures_vals', C.c_void_p), ('textures_widths', C.c_void_p), ('textures_starts', C.c_void_p),
        ('textures_inverse', C.c_void_p),
        ('model', C.c_void_p), ('baked_vals', C.c_void_p),
        ('n_lines_total', C.c_int), ('n_lights_total', C.c_int), ('n_texels_total', C.c_int),
        ('lg_vals', C.c_void_p), ('lg_starts', C.c_void_p), ('lg_geom', C.c_void_p), ('lg_cell', C.c_float),
        ('lg_max_cells', C.c_int), ('lg_list', C.c_void_p), ('lg_pool', C.c_void_p), ('lg_pool_size', C.c_int), ('lg_pool_rows', C.c_void_p),
        ('env_geom', C.c_void_p), ('bake_vis', C.c_void_p), ('bake_vis_starts', C.c_void_p), ('bake_vis_words', C.c_longlong),
        ('wg_cells', C.c_void_p), ('wg_starts', C.c_void_p), ('wg_geom', C.c_void_p), ('wg_cell', C.c_float),
        ('wg_reach_lo', C.c_float), ('wg_reach', C.c_float), ('wg_near', C.c_float), ('wg_pool', C.c_void_p), ('wg_pool_base', C.c_void_p), ('wg_near_rows', C.c_void_p),
        ('model_radius', C.c_float)]


class MsWallGridParent(C.Structure):
    _fields_ = [('cells', C.c_void_p), ('starts', C.c_void_p), ('geom', C.c_void_p), ('cell', C.c_float), ('pool', C.c_void_p)]


class MsAgents(C.Structure):
    _fields_ = [('angles', C.c_void_p), ('positions', C.c_void_p), ('angvelocity', C.c_void_p), ('velocity', C.c_void_p),
                ('headings', C.c_void_p), ('schedule', C.c_void_p)]


class MsMovement(C.Structure):
    _fields_ = [('actions', C.c_void_p), ('table', C.c_void_p), ('n_actions', C.c_int), ('keep', C.c_float)]


class MsStepExtras(C.Structure):
    _fields_ = [('respawn_mask', C.c_void_p), ('respawn_choice', C.c_void_p), ('spawn_positions', C.c_void_p),
                ('spawn_angles', C.c_void_p), ('n_spawns', C.c_int), ('respawn_after', C.c_int),
                ('lifespans', C.c_void_p), ('max_lifespans', C.c_void_p), ('fresh_max', C.c_void_p),
                ('imu', C.c_void_p), ('imu_ang_scale', C.c_float), ('imu_speed_scale', C.c_float)]


class MsSlide(C.Structure):
    _fields_ = [('bounce', C.c_float), ('slid', C.c_void_p), ('stopped', C.c_void_p)]


class MsRender(C.Structure):
    _fields_ = [('indices', C.c_void_p), ('locations', C.c_void_p), ('dots', C.c_void_p), ('distances', C.c_void_p),
                ('screen', C.c_void_p), ('workspace', C.c_void_p), ('obs_rgb', C.c_void_p), ('obs_depth', C.c_void_p),
                ('obs_subsample', C.c_int), ('obs_max_depth', C.c_float), ('obs_centre', C.c_void_p),
                ('seen_stamp', C.c_void_p), ('seen_epoch', C.c_void_p), ('seen_count', C.c_void_p)]


class MsDeathmatch(C.Structure):
    _fields_ = [('centre', C.c_void_p), ('positions', C.c_void_p), ('upper', C.c_void_p), ('clearance', C.c_float), ('hit_damage', C.c_float),
                ('tick_damage', C.c_float), ('health', C.c_void_p), ('damage', C.c_void_p), ('dead', C.c_void_p), ('reset_out', C.c_void_p),
                ('reward', C.c_void_p), ('health_obs', C.c_void_p), ('matchings', C.c_void_p)]


class MsExplorer(C.Structure):
    _fields_ = [('tally', C.c_void_p), ('before', C.c_void_p), ('lengths', C.c_void_p), ('epoch', C.c_void_p), ('over', C.c_void_p),
                ('slack', C.c_int), ('pixels', C.c_int), ('reset_out', C.c_void_p), ('reward', C.c_void_p), ('potential', C.c_void_p),
                ('length_out', C.c_void_p)]


class MsRaycast(C.Structure):
    _fields_ = [('n_rays', C.c_int), ('origins', C.c_void_p), ('dirs', C.c_void_p), ('near_plane', C.c_float),
                ('indices', C.c_void_p), ('locations', C.c_void_p), ('dots', C.c_void_p), ('distances', C.c_void_p),
                ('agents', C.c_void_p), ('grid_rays', C.c_void_p)]


class MsShade(C.Structure):
    _fields_ = [('n_rays', C.c_int), ('indices', C.c_void_p), ('locations', C.c_void_p), ('dots', C.c_void_p), ('screen', C.c_void_p)]


class MsCameraPoses(C.Structure):
    _fields_ = [('n_envs', C.c_int), ('n_cameras', C.c_int), ('res', C.c_int), ('poses', C.c_void_p), ('fov', C.c_float),
                ('projection', C.c_int), ('origins', C.c_void_p), ('dirs', C.c_void_p)]


class MsOverhead(C.Structure):
    _fields_ = [('n_images', C.c_int), ('n_views', C.c_int), ('height', C.c_int), ('width', C.c_int), ('envs', C.c_void_p),
                ('views', C.c_void_p), ('half_width', C.c_float), ('lit', C.c_int), ('background', C.c_float*3),
                ('rgb', C.c_void_p), ('indices', C.c_void_p)]


class MsScenarios(C.Structure):
    _fields_ = [('n_scenarios', C.c_int), ('horizon', C.c_int), ('focal', C.c_int), ('actions', C.c_void_p), ('shared', C.c_int),
                ('base', C.c_void_p), ('table', C.c_void_p), ('n_actions', C.c_int), ('keep', C.c_float), ('mask', C.c_void_p),
                ('positions', C.c_void_p), ('angles', C.c_void_p), ('velocity', C.c_void_p), ('angvelocity', C.c_void_p),
                ('progress', C.c_void_p), ('stops', C.c_void_p), ('first_stop', C.c_void_p), ('trail', C.c_void_p)]


class MsRollouts(C.Structure):
    _fields_ = [('n_candidates', C.c_int), ('horizon', C.c_int), ('actions', C.c_void_p), ('shared_plans', C.c_int), ('table', C.c_void_p),
                ('n_actions', C.c_int), ('keep', C.c_float), ('others', C.c_int), ('mask', C.c_void_p), ('positions', C.c_void_p),
                ('angles', C.c_void_p), ('velocity', C.c_void_p), ('angvelocity', C.c_void_p), ('progress', C.c_void_p), ('stops', C.c_void_p),
                ('first_stop', C.c_void_p), ('trail', C.c_void_p), ('slide', C.c_int), ('bounce', C.c_float), ('slides', C.c_void_p)]


class MsNavGrid(C.Structure):
    _fields_ = [('n_envs', C.c_int), ('cell', C.c_float), ('clearance', C.c_float), ('geom', C.c_void_p), ('starts', C.c_void_p),
                ('max_framed', C.c_int), ('free_cells', C.c_void_p)]


class MsNavFields(C.Structure):
    _fields_ = [('n_goals', C.c_int), ('goals', C.c_void_p), ('mask', C.c_void_p), ('fields', C.c_void_p), ('passes', C.c_void_p)]


class MsNavQuery(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('n_goals', C.c_int),
                ('out', C.c_void_p)]


class MsNavWaypoints(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('goals', C.c_void_p),
                ('n_goals', C.c_int), ('lookahead', C.c_int), ('waypoints', C.c_void_p), ('hops', C.c_void_p)]


class MsNavPaths(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('goals', C.c_void_p),
                ('n_goals', C.c_int), ('max_points', C.c_int), ('paths', C.c_void_p), ('counts', C.c_void_p)]


class MsNavSeedFields(C.Structure):
    _fields_ = [('n_fields', C.c_int), ('marks', C.c_void_p), ('where', C.c_int), ('among', C.c_void_p), ('mask', C.c_void_p),
                ('fields', C.c_void_p), ('passes', C.c_void_p), ('n_seeds', C.c_void_p)]


class MsNavSeedWaypoints(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('n_goals', C.c_int),
                ('lookahead', C.c_int), ('waypoints', C.c_void_p), ('hops', C.c_void_p)]


class MsNavSeedPaths(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('n_goals', C.c_int),
                ('max_points', C.c_int), ('paths', C.c_void_p), ('counts', C.c_void_p)]


class MsNavCostFields(C.Structure):
    _fields_ = MsNavSeedFields._fields_ + [('costs', C.c_void_p), ('n_costs', C.c_int)]


class MsNavCostWaypoints(C.Structure):
    _fields_ = MsNavSeedWaypoints._fields_ + [('costs', C.c_void_p), ('n_costs', C.c_int)]


class MsNavCostPaths(C.Structure):
    _fields_ = MsNavSeedPaths._fields_ + [('costs', C.c_void_p), ('n_costs', C.c_int)]


class MsNavPulls(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('goal', C.c_void_p), ('fields', C.c_void_p), ('goals', C.c_void_p),
                ('n_goals', C.c_int), ('costs', C.c_void_p), ('n_costs', C.c_int), ('reach', C.c_int), ('max_points', C.c_int),
                ('mask', C.c_void_p), ('vertices', C.c_void_p), ('indices', C.c_void_p), ('counts', C.c_void_p), ('cells', C.c_void_p),
                ('lengths', C.c_void_p)]


class MsNavSeen(C.Structure):
    _fields_ = [('n_maps', C.c_int), ('n_viewers', C.c_int), ('n_rays', C.c_int), ('origins', C.c_void_p), ('dirs', C.c_void_p),
                ('distances', C.c_void_p), ('slot', C.c_void_p), ('max_range', C.c_float), ('reset', C.c_void_p), ('countable', C.c_void_p),
                ('maps', C.c_void_p), ('gained', C.c_void_p), ('total', C.c_void_p), ('max_cells', C.c_int)]


class MsNavAges(C.Structure):
    _fields_ = [('n_maps', C.c_int), ('n_viewers', C.c_int), ('n_rays', C.c_int), ('origins', C.c_void_p), ('dirs', C.c_void_p),
                ('distances', C.c_void_p), ('slot', C.c_void_p), ('max_range', C.c_float), ('reset', C.c_void_p), ('countable', C.c_void_p),
                ('advance', C.c_int), ('threshold', C.c_int), ('last', C.c_void_p), ('clock', C.c_void_p), ('swept', C.c_void_p),
                ('gained', C.c_void_p), ('idle', C.c_void_p), ('oldest', C.c_void_p), ('total_age', C.c_void_p), ('n_stale', C.c_void_p),
                ('stale', C.c_void_p), ('ages', C.c_void_p), ('max_cells', C.c_int)]


class MsNavLayer(C.Structure):
    _fields_ = [('values', C.c_void_p), ('is_float', C.c_int), ('n_fields', C.c_int), ('field', C.c_void_p)]


class MsNavChannel(C.Structure):
    _fields_ = [('source', MsNavLayer), ('gate', MsNavLayer), ('where', C.c_int), ('scale', C.c_float), ('outside', C.c_float),
                ('hidden', C.c_float)]


class MsNavWindows(C.Structure):
    _fields_ = [('n_views', C.c_int), ('height', C.c_int), ('width', C.c_int), ('samples', C.c_int), ('views', C.c_void_p),
                ('n_channels', C.c_int), ('channels', C.POINTER(MsNavChannel)), ('out', C.c_void_p)]


class MsNavDraws(C.Structure):
    _fields_ = [('source', MsNavLayer), ('gate', MsNavLayer), ('where', C.c_int), ('lo', C.c_float), ('hi', C.c_float), ('n_sets', C.c_int),
                ('n_draws', C.c_int), ('seed', C.c_ulonglong), ('counter', C.c_void_p), ('mask', C.c_void_p), ('cells', C.c_void_p),
                ('points', C.c_void_p), ('uniforms', C.c_void_p), ('values', C.c_void_p), ('counts', C.c_void_p), ('max_cells', C.c_int)]


class MsNavRegions(C.Structure):
    _fields_ = [('n_fields', C.c_int), ('marks', C.c_void_p), ('where', C.c_int), ('among', C.c_void_p), ('mask', C.c_void_p),
                ('labels', C.c_void_p), ('areas', C.c_void_p), ('counts', C.c_void_p), ('open_cells', C.c_void_p), ('largest', C.c_void_p),
                ('largest_cells', C.c_void_p), ('passes', C.c_void_p)]


class MsNavRegionQuery(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('field', C.c_void_p), ('labels', C.c_void_p), ('n_fields', C.c_int),
                ('labels_at', C.c_void_p)]


class MsNavRegionMasks(C.Structure):
    _fields_ = [('n_requests', C.c_int), ('points', C.c_void_p), ('wanted', C.c_void_p), ('field', C.c_void_p), ('labels', C.c_void_p),
                ('n_fields', C.c_int), ('out', C.c_void_p)]


class MsNavBasins(C.Structure):
    _fields_ = [('n_fields', C.c_int), ('fields', C.c_void_p), ('ids', C.c_void_p), ('n_ids', C.c_int), ('mask', C.c_void_p),
                ('labels', C.c_void_p), ('sizes', C.c_void_p), ('reached', C.c_void_p), ('passes', C.c_void_p)]


class MsNavBasinQuery(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('field', C.c_void_p), ('fields', C.c_void_p), ('labels', C.c_void_p),
                ('n_fields', C.c_int), ('out', C.c_void_p)]


class MsNavPointMarks(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('field', C.c_void_p), ('point_ids', C.c_void_p), ('n_fields', C.c_int),
                ('marks', C.c_void_p), ('ids', C.c_void_p)]


class MsNavZones(C.Structure):
    _fields_ = [('n_fields', C.c_int), ('labels', C.c_void_p), ('n_labels', C.c_int), ('values', C.c_void_p), ('n_values', C.c_int),
                ('marks', C.c_void_p), ('n_marks', C.c_int), ('where', C.c_int), ('within_marks', C.c_int), ('ranked', C.c_int),
                ('max_zones', C.c_int), ('mask', C.c_void_p), ('cells', C.c_void_p), ('marked', C.c_void_p), ('least', C.c_void_p),
                ('nearest', C.c_void_p), ('points', C.c_void_p), ('roots', C.c_void_p), ('n_zones', C.c_void_p)]


class MsNavViews(C.Structure):
    _fields_ = [('n_points', C.c_int), ('points', C.c_void_p), ('headings', C.c_void_p), ('max_range', C.c_float), ('cos_half', C.c_float),
                ('countable', C.c_void_p), ('unseen', C.c_void_p), ('n_maps', C.c_int), ('slot', C.c_void_p), ('mask', C.c_void_p),
                ('values', C.c_void_p), ('counts', C.c_void_p), ('gains', C.c_void_p)]


class MsPercepts(C.Structure):
    _fields_ = [('n_eyes', C.c_int), ('n_points', C.c_int), ('n_nearest', C.c_int), ('eyes', C.c_void_p), ('headings', C.c_void_p),
                ('points', C.c_void_p), ('valid', C.c_void_p), ('pairs', C.c_void_p), ('pairs_shape', C.c_int), ('mask', C.c_void_p),
                ('max_range', C.c_float), ('cos_half', C.c_float), ('visible', C.c_void_p), ('squares', C.c_void_p), ('offsets', C.c_void_p),
                ('counts', C.c_void_p), ('nearest', C.c_void_p), ('near_offsets', C.c_void_p), ('near_distances', C.c_void_p)]


class MsItemCollect(C.Structure):
    _fields_ = [('n_items', C.c_int), ('n_kinds', C.c_int), ('positions', C.c_void_p), ('timers', C.c_void_p), ('kinds', C.c_void_p),
                ('takers', C.c_void_p), ('reset', C.c_void_p), ('reach', C.c_float), ('delay', C.c_int), ('through_walls', C.c_int),
                ('taker', C.c_void_p), ('counts', C.c_void_p), ('due', C.c_void_p)]


class MsItemOverlay(C.Structure):
    _fields_ = [('n_items', C.c_int), ('n_rays', C.c_int), ('n_origins', C.c_int), ('positions', C.c_void_p), ('colors', C.c_void_p),
                ('origins', C.c_void_p), ('dirs', C.c_void_p), ('radius', C.c_float), ('near_plane', C.c_float), ('distances', C.c_void_p),
                ('indices', C.c_void_p), ('locations', C.c_void_p), ('dots', C.c_void_p), ('screen', C.c_void_p), ('items', C.c_void_p)]


class MsNavClearance(C.Structure):
    _fields_ = [('max_range', C.c_float), ('n_radii', C.c_int), ('radii', C.c_float*8), ('max_tiles', C.c_int), ('mask', C.c_void_p),
                ('values', C.c_void_p), ('nearest', C.c_void_p), ('fits', C.c_void_p)]


class MsNavClearQuery(C.Structure):
    _fields_ = [('n_envs', C.c_int), ('n_points', C.c_int), ('points', C.c_void_p), ('skip', C.c_void_p), ('max_range', C.c_float),
                ('mask', C.c_void_p), ('distances', C.c_void_p), ('nearest', C.c_void_p), ('towards', C.c_void_p)]


_int, _flt, _ptr, _p = C.c_int, C.c_float, C.c_void_p, C.POINTER

#: every symbol include/megastep_hip.h (the boundary) and include/megastep_hip_test.h (test hooks) declare, as
#: ``name: (restype, [argtypes])`` - the one place a prototype is written down: lib() binds by it, and tests/test_abi.py holds
#: it against the headers' declarations
PROTOTYPES = {
    'ms_abi_version': (_int, []),
    'ms_strerror': (C.c_char_p, [_int]),
    'ms_last_hip_error': (_int, []),
    'ms_device_count': (_int, []),
    'ms_bake': (_int, [_p(MsScenery), _p(MsConfig), _ptr]),
    'ms_physics': (_int, [_p(MsScenery), _p(MsAgents), _ptr, _p(MsConfig), _ptr]),
    'ms_move_physics': (_int, [_p(MsScenery), _p(MsAgents), _p(MsMovement), _ptr, _p(MsConfig), _ptr]),
    'ms_step_physics': (_int, [_p(MsScenery), _p(MsAgents), _p(MsMovement), _p(MsStepExtras), _ptr, _p(MsConfig), _ptr]),
    'ms_slide_physics': (_int, [_p(MsScenery), _p(MsAgents), _p(MsMovement), _p(MsStepExtras), _p(MsSlide), _ptr, _p(MsConfig), _ptr]),
    'ms_render': (_int, [_p(MsScenery), _p(MsAgents), _p(MsRender), _p(MsConfig), _ptr]),
    'ms_step_render': (_int, [_p(MsScenery), _p(MsAgents), _ptr, _p(MsRender), _p(MsConfig), _ptr]),
    'ms_move_step_render': (_int, [_p(MsScenery), _p(MsAgents), _p(MsMovement), _p(MsStepExtras), _ptr, _p(MsRender), _p(MsConfig), _ptr]),
    'ms_deathmatch_shoot': (_int, [_int, _int, _p(MsDeathmatch), _ptr]),
    'ms_explorer_books': (_int, [_int, _p(MsExplorer), _ptr]),
    'ms_raycast': (_int, [_p(MsScenery), _p(MsAgents), _p(MsRaycast), _p(MsConfig), _ptr]),
    'ms_camera_rays': (_int, [_p(MsAgents), _int, _int, _p(MsConfig), _ptr, _ptr]),
    'ms_shade': (_int, [_p(MsScenery), _p(MsAgents), _p(MsShade), _p(MsConfig), _ptr]),
    'ms_camera_pose_rays': (_int, [_p(MsCameraPoses), _ptr]),
    'ms_overhead': (_int, [_p(MsScenery), _p(MsAgents), _p(MsOverhead), _ptr]),
    'ms_rollouts': (_int, [_p(MsScenery), _p(MsAgents), _p(MsRollouts), _p(MsConfig), _ptr]),
    'ms_scenarios': (_int, [_p(MsScenery), _p(MsAgents), _p(MsScenarios), _p(MsConfig), _ptr]),
    'ms_nav_free': (_int, [_p(MsScenery), _p(MsNavGrid), _ptr]),
    'ms_nav_fields': (_int, [_p(MsNavGrid), _p(MsNavFields), _ptr]),
    'ms_nav_query': (_int, [_p(MsNavGrid), _p(MsNavQuery), _ptr]),
    'ms_nav_waypoints': (_int, [_p(MsNavGrid), _p(MsNavWaypoints), _ptr]),
    'ms_nav_paths': (_int, [_p(MsNavGrid), _p(MsNavPaths), _ptr]),
    'ms_nav_seen': (_int, [_p(MsNavGrid), _p(MsNavSeen), _ptr]),
    'ms_nav_ages': (_int, [_p(MsNavGrid), _p(MsNavAges), _ptr]),
    'ms_nav_windows': (_int, [_p(MsNavGrid), _p(MsNavWindows), _ptr]),
    'ms_nav_draws': (_int, [_p(MsNavGrid), _p(MsNavDraws), _ptr]),
    'ms_nav_regions': (_int, [_p(MsNavGrid), _p(MsNavRegions), _ptr]),
    'ms_nav_region_query': (_int, [_p(MsNavGrid), _p(MsNavRegionQuery), _ptr]),
    'ms_nav_region_masks': (_int, [_p(MsNavGrid), _p(MsNavRegionMasks), _ptr]),
    'ms_nav_views': (_int, [_p(MsScenery), _p(MsNavGrid), _p(MsNavViews), _ptr]),
    'ms_percepts': (_int, [_p(MsScenery), _p(MsPercepts), _ptr]),
    'ms_item_collect': (_int, [_p(MsScenery), _p(MsAgents), _p(MsItemCollect), _ptr]),
    'ms_item_overlay': (_int, [_p(MsScenery), _p(MsItemOverlay), _ptr]),
    'ms_nav_basins': (_int, [_p(MsNavGrid), _p(MsNavBasins), _ptr]),
    'ms_nav_basin_query': (_int, [_p(MsNavGrid), _p(MsNavBasinQuery), _ptr]),
    'ms_nav_point_marks': (_int, [_p(MsNavGrid), _p(MsNavPointMarks), _ptr]),
    'ms_nav_zones': (_int, [_p(MsNavGrid), _p(MsNavZones), _ptr]),
    'ms_nav_clearance': (_int, [_p(MsScenery), _p(MsNavGrid), _p(MsNavClearance), _ptr]),
    'ms_nav_clear_query': (_int, [_p(MsScenery), _p(MsAgents), _p(MsNavClearQuery), _ptr]),
    'ms_nav_seed_fields': (_int, [_p(MsNavGrid), _p(MsNavSeedFields), _ptr]),
    'ms_nav_seed_waypoints': (_int, [_p(MsNavGrid), _p(MsNavSeedWaypoints), _ptr]),
    'ms_nav_seed_paths': (_int, [_p(MsNavGrid), _p(MsNavSeedPaths), _ptr]),
    'ms_nav_cost_fields': (_int, [_p(MsNavGrid), _p(MsNavCostFields), _ptr]),
    'ms_nav_cost_waypoints': (_int, [_p(MsNavGrid), _p(MsNavCostWaypoints), _ptr]),
    'ms_nav_cost_paths': (_int, [_p(MsNavGrid), _p(MsNavCostPaths), _ptr]),
    'ms_nav_pulls': (_int, [_p(MsNavGrid), _p(MsNavPulls), _ptr]),
    'ms_wallgrid_scan':(_int, [_p(MsScenery), _p(MsWallGridParent), _ptr, _int, _int, _ptr, _ptr, _ptr, _ptr]),
    'ms_wallgrid_fill': (_int, [_p(MsScenery), _ptr, _int, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    # the test hooks
    'ms_host_ray_interval': (None, [_f32p, _f32p, _int, _flt, _flt, _int, _i32p, _i32p]),
    'ms_host_ray_interval_wide': (None, [_f32p, _f32p, _int, _flt, _flt, _int, _int, _i32p, _i32p]),
    'ms_debug_ray_groups': (_int, [_int]),
    'ms_debug_physics_pack': (_int, [_int]),
    'ms_debug_last_render_groups': (_int, []),
    'ms_debug_last_step_fused': (_int, []),
    'ms_host_render_plan': (C.c_longlong, [_int, _int, _int, _int, _int, _flt, _int, _i32p]),
    'ms_host_render_block': (_int, [_int, _int, _int, _int, _int, _flt, _int, C.c_longlong, _i32p]),
    'ms_host_physics_pack': (_int, [_int, _int, _int, _int]),
    'ms_debug_render_order': (_int, [_int]),
    'ms_host_order_fans': (_int, [_int, _i32p, _i32p]),
    'ms_debug_ray_group_tail': (_int, [_flt, _int]),
    'ms_debug_pair_telemetry': (_int, [_int]),
    'ms_debug_overhead_cull': (_int, [_int]),
    'ms_host_overhead_keeps': (_int, [_f32p, _int, _int, _int, _int, _flt, _f32p]),
    'ms_host_nav_waypoint': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_path': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_seed_field': (_int, [_ptr, _flt, _ptr, _ptr, _int, _ptr, _int, _ptr, _ptr]),
    'ms_host_nav_seed_waypoint': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_seed_path': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_field_capacity': (_int, [_ptr]),
    'ms_host_nav_cost_field': (_int, [_ptr, _flt, _ptr, _ptr, _int, _ptr, _ptr, _int, _ptr, _ptr]),
    'ms_host_nav_cost_waypoint': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_cost_path': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    'ms_host_nav_cost_capacity': (_int, [_ptr]),
    'ms_debug_nav_cost_variant': (_int, [_int]),
    'ms_host_nav_pull': (_int, [_ptr, _flt, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr, _ptr, _ptr]),
    'ms_debug_nav_pull_scheme': (_int, [_int]),
    'ms_host_nav_seen': (_int, [_ptr, _flt, _ptr, _int, _int, _int, _ptr, _ptr, _ptr, _ptr, _flt, _ptr, _ptr, _ptr, _ptr]),
    'ms_host_nav_ages': (_int, [_ptr, _flt, _p(MsNavAges)]),
    'ms_host_nav_windows': (_int, [_p(MsNavGrid), _p(MsNavWindows)]),
    'ms_host_nav_draws': (_int, [_p(MsNavGrid), _p(MsNavDraws)]),
    'ms_host_nav_regions': (_int, [_p(MsNavGrid), _p(MsNavRegions)]),
    'ms_host_nav_region_query': (_int, [_p(MsNavGrid), _p(MsNavRegionQuery)]),
    'ms_host_nav_region_masks': (_int, [_p(MsNavGrid), _p(MsNavRegionMasks)]),
    'ms_host_nav_region_capacity': (_int, [_ptr]),
    'ms_host_nav_basins': (_int, [_p(MsNavGrid), _p(MsNavBasins)]),
    'ms_host_nav_basin_query': (_int, [_p(MsNavGrid), _p(MsNavBasinQuery)]),
    'ms_host_nav_point_marks': (_int, [_p(MsNavGrid), _p(MsNavPointMarks)]),
    'ms_host_nav_basin_capacity': (_int, [_ptr]),
    'ms_host_nav_zones': (_int, [_p(MsNavGrid), _p(MsNavZones)]),
    'ms_host_nav_views': (_int, [_p(MsNavGrid), _p(MsNavViews), _ptr, _ptr, _int]),
    'ms_host_nav_view_capacity': (_int, []),
    'ms_host_percepts': (_int, [_p(MsPercepts), _int, _ptr, _ptr, _int]),
    'ms_host_item_collect': (_int, [_p(MsItemCollect), _int, _int, _ptr, _ptr, _ptr]),
    'ms_host_item_overlay': (_int, [_p(MsItemOverlay), _int, _ptr]),
    'ms_host_nav_clearance': (_int, [_p(MsNavGrid), _p(MsNavClearance), _ptr, _ptr, _int]),
    'ms_host_nav_clear_folds': (C.c_longlong, [_ptr]),
    'ms_host_nav_clear_chunk': (_int, []),
    'ms_host_nav_clear_query': (_int, [_p(MsNavClearQuery), _ptr, _ptr, _int, _int, _int, _int]),
    'ms_debug_nav_clear_cull': (_int, [_int]),
    'ms_test_arithmetic': (_int, [_ptr]*7 + [C.c_longlong, _ptr]),
    'ms_test_agents_apart': (_int, [_ptr]*4 + [C.c_longlong, _ptr]),
    'ms_test_wall_beyond': (_int, [_ptr]*5 + [C.c_longlong, _ptr]),
    'ms_test_ray_interval': (_int, [_ptr, _ptr, _int, _flt, _flt, _int, _int, _ptr, _ptr, C.c_longlong, _ptr]),
    'ms_test_wedge': (_int, [_ptr]*4 + [C.c_longlong, _ptr]),
    'ms_test_cell_at': (_int, [_ptr]*5 + [C.c_longlong, _ptr]),
    'ms_test_tex_filter': (_int, [_ptr]*6 + [C.c_longlong, _ptr]),
    'ms_test_light_blocked': (_int, [_ptr]*5 + [C.c_longlong, _ptr]),
    'ms_host_lightgrid_cell': (_int, [_ptr, _int, _ptr, _int, _flt, _flt, _int, _int, _flt, _int, _ptr, _ptr, _int]),
    'ms_host_fold_hits': (_int, [_f32p, _i32p, _int, _i32p, _f32p, _i32p]),
    'ms_host_agents_apart': (_int, [_f32p, _f32p, _flt]),
    'ms_host_wall_beyond_reach': (_int, [_f32p, _f32p, _flt]),
    'ms_host_wall_reach': (_flt, [_f32p, _flt]),
    'ms_host_move_velocity': (None, [_flt, _flt, _f32p, _f32p, _f32p]),
    'ms_host_rollouts': (_int, [_ptr, _int, _p(MsAgents), _int, _p(MsRollouts), _p(MsConfig)]),
    'ms_debug_rollout_scheme': (_int, [_int]),
    'ms_host_scenarios': (_int, [_ptr, _int, _p(MsAgents), _int, _p(MsScenarios), _p(MsConfig)]),
    'ms_host_slide': (_int, [_ptr, _ptr, _int, _int, _p(MsAgents), _p(MsMovement), _p(MsStepExtras), _p(MsSlide), _ptr, _p(MsConfig)]),
    'ms_host_shade': (_int, [_p(MsScenery), _p(MsAgents), _p(MsShade)]),
    'ms_host_wall_hidden': (_int, [_flt]*4 + [_f32p, _f32p, _flt]),
    'ms_host_wall_sectors': (None, [_flt]*4 + [_f32p, _i32p, _i32p, _f32p, _i32p]),
    'ms_host_wallgrid_cell': (None, [_ptr, _int, _flt, _flt, _int, _int, _flt, _int, _flt, _flt, _flt, _ptr, _ptr]),
    'ms_host_wall_arc': (None, [_flt]*4 + [_f32p, _i32p, _i32p]),
    'ms_host_wedge': (None, [_flt]*4 + [_i32p, _i32p]),
    'ms_host_wedge_meets': (_int, [_flt]*4 + [_int, _int]),
    'ms_host_sincospi': (None, [_flt, _f32p, _f32p]),
    'ms_host_bake_point_bin': (_int, [_flt]*4),
    'ms_host_bake_wall_bins': (None, [_flt]*6 + [_i32p, _i32p]),
}
SYMBOLS = tuple(PROTOTYPES)


def _source_hash():
    import hashlib
    h = hashlib.sha256()
    import glob
    # (the Makefile's SOURCES, in its order: the translation unit, the kernel files and the host files it includes, the two
    # headers, itself)
    for path in (os.path.join(CSRC, 'megastep_hip.hip'), *sorted(glob.glob(os.path.join(CSRC, 'kernels', '*.h'))),
                 *sorted(glob.glob(os.path.join(CSRC, 'host', '*.h'))), os.path.join(_HERE, '..', 'include', 'megastep_hip.h'), os.path.join(_HERE, '..', 'include', 'megastep_hip_test.h'),
                 os.path.join(CSRC, 'Makefile')):
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False):
    """Compiles csrc/megastep_hip.hip (and the csrc/kernels/*.h and csrc/host/*.h it includes) for gfx950 with hipcc (cross-compiles without a GPU). The library is stale when
    the hash of its sources differs from the one the Makefile recorded next to it (mtimes do not survive copies);
    concurrent callers (one rank per GPU) serialise on a lock file."""
    import fcntl
    stamp = LIB_PATH + '.srchash'
    want = _source_hash()

    def fresh():
        return os.path.exists(LIB_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == want

    if force or not fresh():
        with open(os.path.join(CSRC, '.build.lock'), 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if force or not fresh():                 # (someone else may have built it while we waited)
                import shutil
                hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
                if shutil.which('make') is None or shutil.which(hipcc) is None or not os.access(CSRC, os.W_OK):
                    raise NoToolchain(f'no make / {hipcc} on this host, or {CSRC} is read-only')
                proc = subprocess.run(['make', '-C', CSRC, '-B', 'libmegastep_hip.so'], capture_output=True, text=True)
                if proc.returncode != 0:
                    raise RuntimeError(f'hipcc build of libmegastep_hip.so failed:\n{proc.stdout}\n{proc.stderr}')
    return LIB_PATH


class NoToolchain(OSError):
    """The library cannot be rebuilt here for want of tools (not because its sources do not compile)."""


_lib = None


def lib():
    """The loaded library. (Re)builds the in-tree one first if it is missing or older than its sources; raises if that
    is impossible."""
    global _lib
    if _lib is None:
        if not os.environ.get('MEGASTEP_HIP_LIB'):
            try:
                build()                 # a no-op while the in-tree library matches its sources
            except NoToolchain as e:
                # no hipcc on this host, or a read-only tree: a library that is already there is loaded as it is and
                # the ABI check below decides; without one there is nothing to fall back to.  A compile ERROR is not
                # caught here: sources that do not build must never run a suite against yesterday's kernels.
                if not os.path.exists(LIB_PATH):
                    raise
                import warnings
                warnings.warn(f'{LIB_PATH} could not be rebuilt from the sources next to it ({e}); loading it as it is')
        handle = C.CDLL(LIB_PATH)
        missing = [s for s in SYMBOLS if not hasattr(handle, s)]
        if missing:
            raise ImportError(f'{LIB_PATH} does not export {missing}')
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        if handle.ms_abi_version() != ABI_VERSION:
            raise ImportError(f'{LIB_PATH} has ABI {handle.ms_abi_version()}, this package needs {ABI_VERSION}; rebuild it')
        _lib = handle
    return _lib


def check(code):
    """Turns a negative MS_E* return into a RuntimeError, the way the reference's AT_ASSERTs surface in Python."""
    if code != 0:
        h = lib()
        raise RuntimeError(f'megastep_hip: {h.ms_strerror(code).decode()} (code {code}, hipError {h.ms_last_hip_error()})')


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream(dev):
    """The handle of ``dev``'s current stream, for a launch."""
    # (the current stream's handle straight from torch's C side: torch.cuda.current_stream() builds a Stream object around it
    # first - 5 us of the host's 25 per launch, three launches a step)
    if _raw_stream is not None and dev.index is not None:
        return C.c_void_p(_raw_stream(dev.index))
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _on:
    """Makes ``dev`` the current HIP device for the launch if it is not already."""

    def __init__(self, dev):
        self._guard = None if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self._guard is not None:
            self._guard.__enter__()

    def __exit__(self, *exc):
        if self._guard is not None:
            self._guard.__exit__(*exc)
