"""Shared by tools/pmc_summary.py and tools/sq_summary.py: reading rocprofv3 CSV output of the bench command and
selecting the step-kernel dispatches of the TIMED window (the last 150 turns of the run; the pre-roll, settle and
warm-up launches before them are not part of any reported figure)."""
import csv, glob, json, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel-name tail, turns per launch, step launches in the timed window
FORMS = {"persistent": ("true, false>", 150, 1), "perturn": ("false, false>", 1, 150),
         "caller": ("false, false>", 1, 150),    # caller-supplied orders: per turn the action kernel(s) + the single-turn step kernel
         # learner seat: per turn evg_random_actions_seat + the one-seat instantiation of the single-turn step kernel (evg_step_vs_policy)
         "learner": ("false, false>", 1, 150)}
FORM_KEY = {"persistent": "persistent", "perturn": "one_launch_per_turn", "caller": "caller_actions_per_turn", "learner": "learner_vs_bot_per_turn"}
TWO_KERNEL_FORMS = ("caller", "learner")
ACTION_KERNELS = ("evg_random_actions_kernel", "evg_scripted_actions_kernel")
KERNELS_PER_TURN = 1            # of the caller form: set by the summary scripts (2 for random orders, 3 for two scripted agents)


def kernel_source_hash():
    """the one definition: everglades_amd._lib.kernel_source_hash (what bench.py compares with)"""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import everglades_amd
    return everglades_amd._lib.kernel_source_hash()


OBS_CTYPE = {"float32": "float", "float64": "double", "int16": "short"}
OBS_DTYPE = "float32"          # set by the summary scripts from their command line (the observation type of the profiled run)


def step_kernel(name, form):
    """the step kernel of a launch form: the two-lane kernel evg_step_kernel<OT, 64, MULTI, false> or the four-lane kernel
    evg_step4_kernel<OT, MULTI, WPE> (small batches), whichever the run used"""
    dtype = OBS_CTYPE[OBS_DTYPE]
    multi = FORMS[form][0].split(",")[0]
    if form in TWO_KERNEL_FORMS and any(k in name for k in ACTION_KERNELS):
        return True
    import re
    # evg_step_kernel<OT, 64, MULTI, MT, CHUNKED, SEAT>: the keyed-draw instantiations (MT = false) of the form's MULTI, plain or chunked; the learner form
    # runs SEAT = true
    if form == "learner":
        return re.search(r"evg_step_kernel<%s, 64, false, false, false, true(, 1(, false(, false)?)?)?>" % dtype, name) is not None
    # (round 5: a seventh template parameter, wavefronts per workgroup -- 1 in every product instantiation; then an eighth, the Q form of the one-seat
    # kernel -- false everywhere but in evg_step_vs_policy_smart_q's; then a ninth, the league forms of the one-seat kernel -- false everywhere but in
    # evg_step_vs_league(_q)'s)
    if re.search(r"evg_step_kernel<%s, 64, %s, false, (true|false), false(, 1(, false(, false)?)?)?>" % (dtype, multi), name):
        return True
    return "evg_step4_kernel<%s, %s" % (dtype, multi) in name


# The step-kernel forms the launchers name (csrc/evg_kernels.hip: SingleTurn, Persistent, ...): what each sets of evg_step_kernel's template parameters
# <OT, LPW, MULTI, MT, CHUNKED, SEAT, WPB, QDEC, LEAGUE>, after the observation type
STEP_FORMS = {"single_turn": (64, 0, 0, 0, 0, 1, 0, 0), "persistent": (64, 1, 0, 0, 0, 1, 0, 0), "chunked": (64, 1, 0, 1, 0, 1, 0, 0),
              "stock_entropy": (64, 0, 1, 0, 0, 1, 0, 0), "seat": (64, 0, 0, 0, 1, 1, 0, 0), "seat_q": (64, 0, 0, 0, 1, 1, 1, 0),
              "two_seat_q": (64, 0, 0, 0, 0, 1, 1, 0), "seat_league": (64, 0, 0, 0, 1, 1, 0, 1), "seat_q_league": (64, 0, 0, 0, 1, 1, 1, 1),
              # diagnostic libraries only
              "helper_lanes": (32, 0, 0, 0, 0, 1, 0, 0), "helper_lanes_persistent": (32, 1, 0, 0, 0, 1, 0, 0), "wg256": (64, 0, 0, 0, 0, 4, 0, 0)}
# evg_step_minimized_kernel<OT, LEAGUE> (SeatQMin, SeatQMinLeague): the one-seat Q form's body with the 11-way head
MINIMIZED_FORMS = {"seat_q_min": 0, "seat_q_min_league": 1}
# evg_step_minimized2_kernel<OT, LEAGUE> (TwoSeatQMin, TwoSeatQMinLeague): the two-seat Q form's body with the 11-way head
MINIMIZED2_FORMS = {"two_seat_q_min": 0, "two_seat_q_min_league": 1}
OBS_MANGLED = {"float32": "f", "float64": "d", "int16": "s"}


def step_kernel_symbol(form, obs_dtype="float32"):
    """the mangled symbol of a step-kernel form (a key of STEP_FORMS) for an observation type: what nm, the device assembly and the compiler's
    resource-usage remarks call it"""
    if form in MINIMIZED_FORMS:       # the one-seat Q form with the Minimized agents' 11-way head: a kernel of its own name, <OT, LEAGUE>
        return "_ZN3evg25evg_step_minimized_kernelI%sLb%dEEEvNS_8StepArgsE" % (OBS_MANGLED[obs_dtype], MINIMIZED_FORMS[form])
    if form in MINIMIZED2_FORMS:      # ... and its two-seat form (Minimized self-play), again a kernel of its own name
        return "_ZN3evg26evg_step_minimized2_kernelI%sLb%dEEEvNS_8StepArgsE" % (OBS_MANGLED[obs_dtype], MINIMIZED2_FORMS[form])
    lpw, multi, mt, chunked, seat, wpb, qdec, league = STEP_FORMS[form]
    return "_ZN3evg15evg_step_kernelI%sLi%dELb%dELb%dELb%dELb%dELi%dELb%dELb%dEEEvNS_8StepArgsE" % (OBS_MANGLED[obs_dtype], lpw, multi, mt, chunked, seat, wpb,
                                                                                                         qdec, league)


def counter_rows(directory, form):
    """{counter: [value per dispatch, in dispatch order]} and the matching [duration ns] of the step kernel of `form`."""
    f = glob.glob(os.path.join(directory, "*", "*_counter_collection.csv"))[0]
    per = {}
    meta = {}
    for r in csv.DictReader(open(f)):
        if not step_kernel(r["Kernel_Name"], form):
            continue
        did = int(r["Dispatch_Id"])
        per.setdefault(did, {})[r["Counter_Name"]] = float(r["Counter_Value"])
        meta[did] = dict(ns=int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), grid=int(r["Grid_Size"]), vgpr=int(r["VGPR_Count"]),
                         agpr=int(r["Accum_VGPR_Count"]),
                         sgpr=int(r["SGPR_Count"]), lds=int(r["LDS_Block_Size"]), scratch=int(r["Scratch_Size"]), name=r["Kernel_Name"])
    ids = sorted(per)
    return [per[i] for i in ids], [meta[i] for i in ids]


def timed_window(rows, form):
    """the dispatches of the timed window: the last 150 turns of the run (one step launch each; in the caller form also the action
    kernel(s) of the turn, KERNELS_PER_TURN dispatches per turn in all)"""
    return rows[-FORMS[form][2] * (kernels_per_turn(form)):]


def kernels_per_turn(form):
    return 2 if form == "learner" else (KERNELS_PER_TURN if form == "caller" else 1)


def trace_durations(directory, form):
    """durations (ns) of the step kernel's dispatches, in dispatch order, from a --kernel-trace CSV"""
    f = glob.glob(os.path.join(directory, "*", "*_kernel_trace.csv"))[0]
    rows = [(int(r["Dispatch_Id"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(open(f)) if step_kernel(r["Kernel_Name"],
                                                                                                                                         form)]
    return [d for _, d in sorted(rows)]
