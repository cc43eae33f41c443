"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/knob_cfgs.json: what the three plan-cfg builders (engine.native_cfg,
native_khead_cfg, native_neck_cfg) make of every PH_* variable they read, value by value, at one small geometry.  The file is
the record of the commit BEFORE the variables moved into polyphonicformer_amd/knobs.py (run there, once); tests/test_knobs_host.py
runs the same grid (`run_grid`) on the current tree and expects no difference.  Needs neither a GPU nor libpolyhead.so.
Run:  PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_knobs.py"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# every variable a cfg builder reads, and PH_VIDEO_SLOT_PRIO as the one that must reach none of them
VARIABLES = ("PH_CONV_POOLX", "PH_CONV_UP2", "PH_POOL_NSPLIT", "PH_POOLX_NSPLIT", "PH_UP2_SHARED_WGS", "PH_KHEAD_TWOPASS",
             "PH_NECK_OUT2", "PH_NECK_C16", "PH_NECK_STREAMS", "PH_VIDEO_SLOT_PRIO")
VALUES = (None, "", "0", "1", "2", "3", "7", "x")            # None: unset
EXTRA_VALUES = {"PH_VIDEO_SLOT_PRIO": ("low",)}
B, N, H, W = 2, 16, 12, 20
NECK_SHAPES = ((12, 20), (6, 10), (3, 5), (2, 3))


def builders():
    """{label: zero-argument call}: each builder plain, and with every explicit argument that meets a variable"""
    from polyphonicformer_amd import engine as E
    dec = lambda **kw: E.native_cfg(B, N, H, W, 3, 19, 2048, "mixed16", **kw)
    kh = lambda **kw: E.native_khead_cfg(B, H, W, N, 19, 8, True, 32, "fp16", **kw)
    neck = lambda **kw: E.native_neck_cfg(B, NECK_SHAPES, 32, "fp16", **kw)
    return {
        "native_cfg": dec, "native_cfg(nsplit=5)": lambda: dec(nsplit=5), "native_cfg(frame_invariant)": lambda: dec(frame_invariant=True),
        "native_khead_cfg": kh, "native_khead_cfg(onepass=True)": lambda: kh(onepass=True),
        "native_khead_cfg(onepass=False)": lambda: kh(onepass=False), "native_khead_cfg(nsplit=5)": lambda: kh(nsplit=5),
        "native_neck_cfg": neck, "native_neck_cfg(fused_out=True)": lambda: neck(fused_out=True),
        "native_neck_cfg(fused_out=False)": lambda: neck(fused_out=False), "native_neck_cfg(c16=False)": lambda: neck(c16=False),
        "native_neck_cfg(c16=True)": lambda: neck(c16=True), "native_neck_cfg(tower_streams=False)": lambda: neck(tower_streams=False),
        "native_neck_cfg(tower_streams='always')": lambda: neck(tower_streams="always"),
    }


def run_grid():
    """[[builder label, variable, value or None, bytes(cfg).hex() or the raised exception's type name]] with ONLY that variable of
    VARIABLES set; the caller's environment is put back"""
    saved = {v: os.environ.pop(v, None) for v in VARIABLES}
    rows = []
    try:
        calls = builders()
        for var in VARIABLES:
            for val in VALUES + EXTRA_VALUES.get(var, ()):
                if val is not None:
                    os.environ[var] = val
                for label, call in calls.items():
                    try:
                        got = bytes(call()).hex()
                    except Exception as e:                   # noqa: BLE001 -- the type IS the record
                        got = type(e).__name__
                    rows.append([label, var, val, got])
                os.environ.pop(var, None)
    finally:
        for v, old in saved.items():
            if old is not None:
                os.environ[v] = old
    return rows


def pack(rows):
    """the file's form: every distinct outcome once, the rows point at it"""
    outcomes = sorted({r[3] for r in rows})
    at = {o: i for i, o in enumerate(outcomes)}
    return dict(geometry=dict(B=B, N=N, H=H, W=W, neck_shapes=NECK_SHAPES), outcomes=outcomes, rows=[r[:3] + [at[r[3]]] for r in rows])


def unpack(doc):
    return [r[:3] + [doc["outcomes"][r[3]]] for r in doc["rows"]]


PATH = os.path.join(REPO, "tests", "golden", "knob_cfgs.json")


def main():
    rows = run_grid()
    with open(PATH, "w") as f:
        json.dump(pack(rows), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", PATH, len(rows), "rows,", len({r[3] for r in rows}), "distinct outcomes,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
