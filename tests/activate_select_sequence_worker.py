"""One reference leg of the key-frame sequence WITH the distance map (adp_set_distance_map) in a process of its own, for the reference-against-itself yardstick
of tests/test_activate_select_gpu.py: the library pair is chosen by LDSO_REF_LIB / LDSO_ADAPTER_LIB in the environment (as tests/ref_sequence_worker.py).
    python tests/activate_select_sequence_worker.py <config> <K> <multithreading 0|1> <out.pkl> <per_frame> <desired point density>"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    cfg, K, mt, out, per_frame, density = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), float(sys.argv[6])
    from ldso_amd import synth
    import activation_select_common as asc
    from adapter_sequence_common import run_sequence
    win = synth.make_config(cfg, extra_frames=K)
    asc.set_desired_point_density(density)
    asc.set_distance_map(True)
    r, log = run_sequence(win, K, multithreading=bool(mt), per_frame=per_frame)
    with open(out, "wb") as f:
        pickle.dump(dict(log=log, trace=asc.min_act_dist_trace()), f)
    r.close()


if __name__ == "__main__":
    main()
