"""Command line front-end -- the reference's `cli.py --inverse-kine` contract.

    python -m inversekinematicsann_amd.cli --inverse-kine --method fabrik --points P.csv \
        [--to-file OUT.csv] [--verbose] [--tol 1e-3] [--max-iter 100]
    python -m inversekinematicsann_amd.cli --inverse-kine --method ann --model M.h5 \
        --points P.csv [--to-file OUT.csv] [--verbose]

Same flags, outputs and error behaviour as cli.py:232-388 of the reference:
the points CSV is read with pandas (header row, x,y,z columns), angles are
written as theta1..theta4 (index=False); OutOfRobotReachException and
ValueError are printed and the command still exits 0 (cli.py:250-252, 300),
a ZeroDivisionError propagates.  Plotting (plot/plot.py) is out of scope:
--verbose prints the angles and the FK round-trip error instead of plotting.
Extra flags: --tol / --max-iter (FABRIK, defaults 1e-3 / 100 as the
reference's constructor), --device, and for --method ann --refine-tol FLOAT
[--refine-iter INT, default 20]: the network's angles are polished on the GPU by
the damped-least-squares refine (kinematics/refine.py) and written as float64;
--verbose then reports the network's and the polished FK error.  With --refine-tol,
--joint-limits="lo:hi,lo:hi,,lo:hi" (radians, an empty field for a free joint) keeps
the polished angles inside the robot's joint limits; --verbose adds how many points
ended on a limit and how many did not converge.
`--method analytic [--pitch FLOAT] [--elbow up|down] [--nearest-pitch]` (not in the
reference) solves in closed form at a chosen tool pitch theta2 + theta3 + theta4 and
elbow branch (kinematics/analytic.py); a fourth CSV column `pitch` gives one pitch per
point; --verbose then reports the FK round trip and how many pitches were moved.
`--generate-data --shape {circle,cube,cube_random,random,spring,random_dist}` runs
the reference's generators (robot/position_generator.py, cli.py:80-229) with the
same arguments: --to-file writes the x,y,z CSV, --verbose prints the shape's
parameters as the reference does (its 3-D plot is out of scope).
`--method chain --dh FILE [--seed-angles FILE] [--joint-limits=...] [--restarts R]
[--refine-tol FLOAT | --tol FLOAT] [--max-iter INT]` (not in the reference) solves any DH
chain of 2..8 revolute joints by damped least squares with restarts
(kinematics/chain.py): FILE is a CSV of four lines (theta, d, a, alpha) with one value
per joint and no header, the theta line being the home pose that seeds a solve
without --seed-angles (a CSV with a header row, one angle row per point);
--joint-limits takes one field per joint here; the angles are written as
theta1..thetaN.  Defaults: tol 1e-6, 60 steps an attempt, 4 restarts.
`--method chain --poses FILE [--rot-tol FLOAT] [--rot-weight FLOAT]` takes tool poses in
place of --points: a CSV with the header x,y,z,r11,r12,r13,r21,...,r33, the position and
the rotation matrix row by row (ChainInverseKinematics.ikine_pose); --rot-tol (default:
the tolerance) bounds the rotation error sqrt(1/2 |R - G|_F^2) of a solved pose,
--rot-weight (default 1) weighs the rotation rows of the step; --verbose adds the
largest rotation error.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

EXAMPLES = {
    "ann": "--inverse-kine --method ann --model model_filename.h5 --points filename.csv",
    "fabrik": "--inverse-kine --method fabrik --points filename.csv",
    "analytic": "--inverse-kine --method analytic --points filename.csv --pitch -1.5708 "
                "--elbow up --nearest-pitch",
    "chain": "--inverse-kine --method chain --dh dh_table.csv --points filename.csv "
             "--joint-limits=-1.5:1.5,,,,, --restarts 4",
    "circle": "--generate-data --shape circle --radius 3 --samples 20 --center 1,5,2",
    "cube": "--generate-data --shape cube --step 0.75 --dim 2,3,4 --start 1,2,3",
    "cube_random": "--generate-data --shape cube_random --step 0.75 --dim 2,3,4 --start 1,2,3",
    "random": "--generate-data --shape random --limits 0,3;0,4;0,5 --samples 20",
    "spring": "--generate-data --shape spring --samples 50 --dim 2,3,6",
    "random_dist": "--generate-data --shape random_dist --dist normal --samples 100 "
                   "--std_dev 0.35 --limits 0,3;0,4;0,5",
}
# each shape's required arguments (cli.py:91-94, 117-119, 155-157, 182-184, 206-211)
SHAPE_ARGS = {"circle": ("radius", "samples", "center"), "cube": ("step", "dim", "start"),
              "cube_random": ("step", "dim", "start"), "random": ("samples", "limits"),
              "spring": ("samples", "dim"),
              "random_dist": ("dist", "samples", "std_dev", "limits")}


def _parser():
    p = argparse.ArgumentParser(prog="cli")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--inverse-kine", action="store_true")
    g.add_argument("--generate-data", action="store_true")
    p.add_argument("--method", choices=["ann", "fabrik", "analytic", "chain"])
    p.add_argument("--shape", choices=list(SHAPE_ARGS))
    p.add_argument("--example", action="store_true")
    p.add_argument("--points", type=str, help=".csv file name with stored trajectory points")
    p.add_argument("--model", type=str, help="select saved model .h5 (or .npz) filename")
    p.add_argument("--to-file", type=str)
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--show-path", action="store_true")
    p.add_argument("--separate-plots", action="store_true")
    p.add_argument("--tol", type=float, default=None,
                   help="FABRIK error margin (default 0.001); chain: the tolerance (default 1e-6)")
    p.add_argument("--max-iter", type=int, default=None,
                   help="FABRIK iteration cap (default 100); chain: steps of one attempt "
                        "(default 60)")
    p.add_argument("--dh", type=str, help="chain: CSV of four lines theta, d, a, alpha")
    p.add_argument("--seed-angles", type=str, help="chain: CSV of one seed row per point")
    p.add_argument("--restarts", type=int, default=None, help="chain: restarts (default 4)")
    p.add_argument("--poses", type=str,
                   help="chain: CSV x,y,z,r11,..,r33 of tool poses, in place of --points")
    p.add_argument("--rot-tol", type=float, default=None,
                   help="chain with --poses: the rotation tolerance (default: the tolerance)")
    p.add_argument("--rot-weight", type=float, default=None,
                   help="chain with --poses: weight of the rotation rows (default 1)")
    p.add_argument("--device", type=int, default=None, help="GPU index")
    p.add_argument("--refine-tol", type=float, default=None,
                   help="ANN: polish the angles until |FK(theta) - p| <= this")
    p.add_argument("--refine-iter", type=int, default=20, help="ANN: refine step cap")
    p.add_argument("--joint-limits", type=str, default=None,
                   help='ANN with --refine-tol: "lo:hi,lo:hi,,lo:hi" in radians, one field per '
                        'joint, an empty field for a free joint (write --joint-limits=... when '
                        'the first bound is negative)')
    p.add_argument("--pitch", type=float, default=None,
                   help="analytic: tool pitch theta2 + theta3 + theta4 of every point (radians)")
    p.add_argument("--elbow", choices=["up", "down"], default=None,
                   help="analytic: elbow branch (default up, theta3 <= 0)")
    p.add_argument("--nearest-pitch", action="store_true",
                   help="analytic: move an unreachable pitch to the nearest reachable one")
    # data generators
    p.add_argument("--samples", type=int)
    p.add_argument("--dim", type=str)
    p.add_argument("--dist", type=str, choices=["normal", "uniform", "random"])
    p.add_argument("--std_dev", type=float)
    p.add_argument("--limits", type=str)
    p.add_argument("--radius", type=float)
    p.add_argument("--center", type=str)
    p.add_argument("--step", type=float)
    p.add_argument("--start", type=str)
    return p


def _read_points(path):
    import pandas as pd
    return pd.read_csv(path).values.tolist()


def _read_points_pitch(path):
    """(points, per-point pitches or None): a fourth column `pitch` is split off."""
    import pandas as pd
    df = pd.read_csv(path)
    if "pitch" not in df.columns:
        return df.values.tolist(), None
    return df.drop(columns="pitch").values.tolist(), df["pitch"].to_numpy(np.float64)


def _save_angles(data, filename, nj=4):
    import pandas as pd
    pd.DataFrame(data, columns=[f'theta{i + 1}' for i in range(nj)]).to_csv(filename, index=False)


def _verbose(points, joint_angles):
    from .kinematics.forward import ForwardKinematics
    from .robot.robot import SixDOFRobot as Robot
    fk = ForwardKinematics([list(r) for r in Robot.dh_matrix])
    xyz = fk.fkine_batch(np.asarray(joint_angles, np.float64))
    err = np.linalg.norm(xyz - np.asarray(points, np.float64), axis=1)
    print(joint_angles)
    print(f"FK round trip: max |FK(theta) - p| = {err.max():.6g}, mean = {err.mean():.6g} "
          f"over {len(err)} points")


def _joint_limits(text, parser, nj=4):
    """--joint-limits "lo:hi,lo:hi,,lo:hi": nj entries, (lo, hi) or None."""
    fields = text.split(",")
    if len(fields) != nj:
        parser.error(f"--joint-limits takes {nj} comma-separated fields, got {len(fields)}")
    out = []
    for i, f in enumerate(fields):
        if not f.strip():
            out.append(None)
            continue
        try:
            lo, hi = (float(v) for v in f.split(":"))
        except ValueError:
            parser.error(f"--joint-limits: joint {i + 1}: expected lo:hi, got {f!r}")
        out.append((lo, hi))
    return out


POSE_COLUMNS = ["x", "y", "z"] + [f"r{i}{j}" for i in (1, 2, 3) for j in (1, 2, 3)]


def _read_poses(path, parser):
    """--poses: (points n x 3, rotations n x 3 x 3) of a CSV with POSE_COLUMNS."""
    import pandas as pd
    df = pd.read_csv(path)
    if list(df.columns) != POSE_COLUMNS:
        parser.error("--poses: the header must be " + ",".join(POSE_COLUMNS))
    v = df.to_numpy(np.float64)
    return v[:, :3].copy(), v[:, 3:].reshape(-1, 3, 3).copy()


def _chain(args, parser):
    """--method chain: ChainInverseKinematics on the table of --dh."""
    from .kinematics.chain import ChainInverseKinematics, chain_dh, chain_fk, chain_limit_arrays
    from .robot.robot import OutOfRobotReachException
    if args.dh is None:
        parser.error("the following arguments are required: --dh")
    for flag, given in (("--model", args.model is not None), ("--pitch", args.pitch is not None),
                        ("--elbow", args.elbow is not None), ("--nearest-pitch", args.nearest_pitch)):
        if given:
            parser.error(f"{flag} is not valid with --method chain")
    if args.refine_tol is not None and args.tol is not None:
        parser.error("--method chain takes --refine-tol or --tol, not both")
    if args.poses is not None and args.points is not None:
        parser.error("--method chain takes --points or --poses, not both")
    for flag, given in (("--rot-tol", args.rot_tol is not None),
                        ("--rot-weight", args.rot_weight is not None)):
        if given and args.poses is None:
            parser.error(f"{flag} is only valid with --poses")
    if args.rot_tol is not None and np.isnan(args.rot_tol):
        parser.error("--rot-tol takes a number")
    if args.rot_weight is not None and not (np.isfinite(args.rot_weight) and args.rot_weight >= 0):
        parser.error("--rot-weight takes a finite number >= 0")
    try:
        dh = chain_dh(np.loadtxt(args.dh, delimiter=",", ndmin=2))
    except (OSError, ValueError) as e:
        parser.error(f"--dh: {e}")
    nj = dh.shape[1]
    joint_limits = None
    if args.joint_limits is not None:
        joint_limits = _joint_limits(args.joint_limits, parser, nj)
        try:
            chain_limit_arrays(joint_limits, nj)
        except ValueError as e:
            parser.error(f"--joint-limits: {e}")
    restarts = 4 if args.restarts is None else args.restarts
    if not 0 <= restarts <= 255:
        parser.error("--restarts takes 0..255")
    tol = args.refine_tol if args.refine_tol is not None else args.tol
    if args.poses is not None:
        points, rotations = _read_poses(args.poses, parser)
    else:
        points = _read_points(args.points)
    seed = None
    if args.seed_angles is not None:
        import pandas as pd
        seed = pd.read_csv(args.seed_angles).to_numpy(np.float64)
        if seed.shape != (len(points), nj):
            parser.error(f"--seed-angles: {seed.shape[0]} rows of {seed.shape[1]} angles for "
                         f"{len(points)} points of {nj} joints")
    ik = ChainInverseKinematics(dh, joint_limits, tol=1e-6 if tol is None else tol,
                                max_iter=60 if args.max_iter is None else args.max_iter,
                                restarts=restarts, rot_tol=args.rot_tol,
                                rot_weight=1.0 if args.rot_weight is None else args.rot_weight)
    try:
        if args.poses is not None:
            joint_angles = ik.ikine_pose((points, rotations), seed)
        else:
            joint_angles = ik.ikine(points, seed)
    except (OutOfRobotReachException, ValueError) as kine_exception:
        print(str(kine_exception))
        return 0
    if args.verbose:
        err = np.linalg.norm(chain_fk(dh, joint_angles) - np.asarray(points, np.float64), axis=1)
        it, tries = ik.last_iters, ik.last_tries
        print(joint_angles)
        print(f"FK round trip: max |FK(theta) - p| = {err.max():.6g}, mean = {err.mean():.6g} "
              f"over {len(err)} points")
        print(f"chain: {nj} joints, tol {ik.tol:g}, max {int(it.max())} steps (mean "
              f"{it.mean():.3g}), {int((tries > 0).sum())} points solved by a restart, "
              f"{ik.last_stats.n_capped} not converged")
        if args.poses is not None:
            print(f"rotation error: max sqrt(1/2 |R - G|_F^2) = {np.nanmax(ik.last_rot_err):.6g} "
                  f"(rot-tol {ik.rot_tol:g}, rot-weight {ik.rot_weight:g})")
    if args.to_file is not None:
        _save_angles(joint_angles, args.to_file, nj)
    return 0


def _ikine(args, parser):
    from .robot.robot import OutOfRobotReachException
    from .robot.robot import SixDOFRobot as Robot
    if args.method is None:
        parser.error("the following arguments are required: --method")
    if args.example:
        print(EXAMPLES[args.method])
        return 0
    if args.points is None and not (args.method == "chain" and args.poses is not None):
        parser.error("the following arguments are required: --points")
    if args.method == "chain":
        return _chain(args, parser)
    for flag, given in (("--dh", args.dh is not None), ("--seed-angles", args.seed_angles is not None),
                        ("--restarts", args.restarts is not None), ("--poses", args.poses is not None),
                        ("--rot-tol", args.rot_tol is not None),
                        ("--rot-weight", args.rot_weight is not None)):
        if given:
            parser.error(f"{flag} is only valid with --method chain")
    if args.method == "ann" and args.model is None:
        parser.error("the following arguments are required: --model")
    if args.refine_tol is not None and args.method != "ann":
        parser.error("--refine-tol is only valid with --method ann")
    joint_limits = None
    if args.joint_limits is not None:
        if args.method != "ann" or args.refine_tol is None:
            parser.error("--joint-limits is only valid with --method ann --refine-tol")
        joint_limits = _joint_limits(args.joint_limits, parser)
        from .kinematics.refine import joint_limit_arrays
        try:
            joint_limit_arrays(joint_limits)
        except ValueError as e:
            parser.error(f"--joint-limits: {e}")
    if args.method != "analytic":
        for flag, given in (("--pitch", args.pitch is not None), ("--elbow", args.elbow is not None),
                            ("--nearest-pitch", args.nearest_pitch)):
            if given:
                parser.error(f"{flag} is only valid with --method analytic")
    from .kinematics.inverse import AnalyticInverseKinematics, AnnInverseKinematics, \
        FabrikInverseKinematics
    dh = [list(r) for r in Robot.dh_matrix]
    if args.method == "analytic":
        points, pitches = _read_points_pitch(args.points)
        if pitches is not None and args.pitch is not None:
            parser.error("--pitch is not valid with a points file that has a pitch column")
        ik = AnalyticInverseKinematics(dh, Robot.links_lengths, Robot.effector_workspace_limits,
                                       pitch=args.pitch if pitches is None else pitches,
                                       elbow=args.elbow or "up", nearest=args.nearest_pitch)
    else:
        points = _read_points(args.points)
    if args.method == "ann":
        refine = (None if args.refine_tol is None
                  else {"tol": args.refine_tol, "max_iter": args.refine_iter})
        ik = AnnInverseKinematics(dh, Robot.links_lengths, Robot.effector_workspace_limits,
                                  refine=refine, joint_limits=joint_limits)
        ik.load_model(args.model)
    elif args.method == "fabrik":
        ik = FabrikInverseKinematics(dh, Robot.links_lengths, Robot.effector_workspace_limits,
                                     0.001 if args.tol is None else args.tol,
                                     100 if args.max_iter is None else args.max_iter)
    try:
        joint_angles = ik.ikine(points)
    except (OutOfRobotReachException, ValueError) as kine_exception:
        print(str(kine_exception))
        return 0
    if args.verbose:
        _verbose(points, joint_angles)
        if args.refine_tol is not None:
            seed, it = ik.last_seed_fk_err, ik.last_iterations
            print(f"ANN seed: max |FK(theta) - p| = {seed.max():.6g}, mean = {seed.mean():.6g}; "
                  f"refined to tol {args.refine_tol:g} in max {int(it.max())} steps "
                  f"(mean {it.mean():.3g}), {ik.last_stats.n_capped} of {len(it)} points not "
                  "converged")
            if joint_limits is not None:
                lo, hi = ik.joint_limits
                ang = np.asarray(joint_angles, np.float64)
                at = int(((ang == lo) | (ang == hi)).any(axis=1).sum())
                print(f"joint limits: {at} of {len(it)} points at a limit, "
                      f"{ik.last_stats.n_capped} not converged")
        if args.method == "analytic":
            print(f"analytic: max |FK(theta) - p| = {np.nanmax(ik.last_fk_err):.6g} (in the solve's "
                  f"launch), {ik.last_stats.n_capped} of {len(points)} pitches moved")
    if args.to_file is not None:
        _save_angles(joint_angles, args.to_file)
    return 0


def _floats(text):
    return [float(v) for v in text.split(",")]


def _limits(text):
    lim = text.split(";")
    return {"x": _floats(lim[0]), "y": _floats(lim[1]), "z": _floats(lim[2])}


def _generate(args, parser):
    """cli.py:80-229: the shape's generator on its arguments; --verbose prints the
    arguments tuple (the reference's ShapeCommand.verbose, before its plot),
    --to-file the points as an x,y,z CSV."""
    import pandas as pd
    from .robot import position_generator as G
    if args.shape is None:
        parser.error("the following arguments are required: --shape")
    if args.example:
        print(EXAMPLES[args.shape])
        return 0
    missing = [a for a in SHAPE_ARGS[args.shape] if getattr(args, a) is None]
    if missing:
        parser.error("the following arguments are required: " +
                     ", ".join("--" + a for a in missing))
    sh = args.shape
    if sh == "circle":
        center = _floats(args.center)
        params = (args.radius, args.samples, center)
        pts = G.circle(args.radius, args.samples, center)
    elif sh in ("cube", "cube_random"):
        dim, start = _floats(args.dim), _floats(args.start)
        params = (args.step, dim, start)
        pts = (G.cube if sh == "cube" else G.cube_random)(args.step, *dim, start)
    elif sh == "random":
        lim = _limits(args.limits)
        params = (args.samples, lim)
        pts = G.random(args.samples, lim)
    elif sh == "spring":
        dim = _floats(args.dim)
        params = (args.samples, *dim)
        pts = G.spring(args.samples, *dim)
    else:
        lim = _limits(args.limits)
        params = (args.samples, lim, args.dist, args.std_dev)
        pts = G.random_distribution(args.samples, lim, args.dist, args.std_dev)
    if args.verbose:
        print(params)
    if args.to_file is not None:
        pd.DataFrame(pts.tolist(), columns=["x", "y", "z"]).to_csv(args.to_file, index=False)
    return 0


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if args.device is not None:
        os.environ["IKHIP_DEVICE"] = str(args.device)
    if not args.inverse_kine and not args.generate_data:
        parser.error('Operation --inverse-kine or --generate-data must be choosed')
    if args.inverse_kine:
        return _ikine(args, parser)
    return _generate(args, parser)


if __name__ == "__main__":
    sys.exit(main())
