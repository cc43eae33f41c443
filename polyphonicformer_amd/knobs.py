"""The PH_* variables of the Python side: one table (`KNOBS`), one reader (`get`), one printed list (`python -m
polyphonicformer_amd.knobs`, the table of DESIGN.md section 7g).  No other module of the package looks at the process's
variables.  Standard library only: `_lib` and `build` import this module.

`get` reads the variable at the time of the call and caches nothing, so whoever sets one (a test's monkeypatch, bench.py)
is seen by the next plan-cfg build.  The library's own switches are a different table with a different life (read once, then
set by call: `_lib.switches`, include/polyhead.h PH_SWITCH_*)."""
import collections
import os

# kind: how `get` parses the text --
#   "flag": bool, set and non-empty = on            "int" : int, or None when unset or empty; anything else ValueError
#   "text": the text, `default` when unset          "raw" : the text as it is, "" when unset
# effect: "plan cfg" (read by `reader` whenever it builds a plan's cfg struct: engine.native_cfg / native_khead_cfg /
#   native_neck_cfg, whose plans the module caches key by that cfg), "import" (read once, when `reader` is imported),
#   "video" (read by VideoStreamRunner as it runs), "build" (read when the library is compiled)
Knob = collections.namedtuple("Knob", "name kind default effect reader doc")

KNOBS = {k.name: k for k in (
    Knob("PH_QUERY_FULL_SPLIT", "flag", False, "import", "engine.MODES",
         "`mixed16` / `fp16` run the all-hi/lo query kernels instead of the hybrid ones (§4.3c)"),
    Knob("PH_CONV_POOLX", "text", "auto", "plan cfg", "engine.native_cfg",
         "`0` never / `1` wherever it exists: the stage-boundary conv also pools (`ph_dynconv_poolx`); anything else: the library's rule"),
    Knob("PH_CONV_UP2", "text", "auto", "plan cfg", "engine.native_cfg",
         "`0` never / `1` wherever it exists: final stage as `ph_dynconv_up2`; anything else: the library's rule (fused from B·H ≥ 512, §4.4b)"),
    Knob("PH_POOL_PAIR", "text", "1", "import", "engine.POOL_PAIR",
         "`0`: the last two stages pool depth_feats in a launch each; anything else: in one paired launch where "
         "`ph_pool_depth_pair_supported` (`DecodePlan` with the fused conv + pooling and S ≥ 3, §4.2; same bits either way)"),
    Knob("PH_POOL_NSPLIT", "int", None, "plan cfg", "engine.native_cfg, native_khead_cfg, default_nsplit",
         "pixel ranges of the pooling kernels (cfg field `nsplit`; an `nsplit` argument wins).  Known oddity: `0` means the "
         "library's rule in the cfg builders, while `engine.default_nsplit` returns the 0"),
    Knob("PH_POOLX_NSPLIT", "int", None, "plan cfg", "engine.native_cfg",
         "pixel ranges of the fused conv + pooling (cfg field `nsplit_px`); not read for a `frame_invariant` plan"),
    Knob("PH_UP2_SHARED_WGS", "int", None, "plan cfg", "engine.native_cfg",
         "workgroups of the fused final-stage kernel of a plan that `shares_gpu` (default 1.5 per CU: 0 … +1.3 % on the step, "
         "`profiles/r06/knob_sweep.txt`)"),
    Knob("PH_KHEAD_TWOPASS", "flag", False, "plan cfg", "engine.native_khead_cfg",
         "KernelHead post-neck by `ph_khead_fused` (two passes) instead of `ph_khead_onepass` (§4.5b; cfg field `onepass`); "
         "an `onepass=True` argument beside it is an error"),
    Knob("PH_NECK_OUT2", "text", "1", "plan cfg", "engine.native_neck_cfg",
         "`0`: the neck's three output convs per map (round 3's form; cfg field `fused_out`); `2` / `3`: removed measurement "
         "forms, refused; anything else: the library's rule"),
    Knob("PH_NECK_C16", "text", "1", "plan cfg", "engine.native_neck_cfg",
         "`0`: no channels-last planes into level 0's stride-2 conv (cfg field `c16`)"),
    Knob("PH_NECK_STREAMS", "text", "1", "plan cfg", "engine.native_neck_cfg",
         "`0` never / `2` always: the four level towers on their own streams (cfg field `tower_buffers`); anything else: from 4 frames"),
    Knob("PH_VIDEO_API_EAGER", "flag", False, "video", "video (the module API's simple_test)",
         "the per-frame module call launches its heads eagerly instead of replaying a one-slot `VideoStreamRunner` graph"),
    Knob("PH_VIDEO_HOST_SELECT", "flag", False, "video", "video.VideoStreamRunner",
         "the merge's candidate selection on the host, the module API's form (the default of `device_select`: on the device)"),
    Knob("PH_VIDEO_SLOT_PRIO", "text", "", "video", "video.VideoStreamRunner",
         "`low`: the slots' head streams one priority level below the caller's stream; anything else: the same priority"),
    Knob("PH_VIDEO_BORROW", "text", "1", "video", "video.VideoStreamRunner",
         "`0`: every launch copies its frames into slot-owned buffers, none reads the caller's tensors"),
    Knob("PH_VIDEO_CLIP_TOWERS", "text", "1", "video", "video.VideoStreamRunner",
         "neck level towers on their own streams inside the slots' graphs: `0` never, `2` also in the sequential one-frame "
         "loop, anything else from 2 frames per launch"),
    Knob("PH_VIDEO_CLIP_BATCH", "int", None, "video", "video.VideoStreamRunner",
         "frames per heads launch of a clip (unset, empty or 0: half the clip, at most 8; 1: one frame per launch)"),
    Knob("PH_ALT_LIB", "raw", "", "import", "_lib",
         "path of a variant build of libpolyhead.so to load instead (`tools/build_variant.py`, same-box A/B timing)"),
    Knob("PH_EXTRA_HIPCC_FLAGS", "raw", "", "build", "build.build_library",
         "extra hipcc arguments for every source, e.g. `-DK1_TIMELINE` (phase stamps of the one-pass kernel; right results, costs registers)"),
)}


_UNSET = {k.name: k.default for k in KNOBS.values()}        # what `get` needs of a row, as plain dicts
_KIND = {k.name: k.kind for k in KNOBS.values()}


def get(name, _environ=os.environ):
    """the variable's value now, parsed by its row's kind; KeyError for a name the table does not hold.  The cfg builders call
    this on every forward of the module API, nearly always for an unset variable, so that path is the mapping's own subscript
    (its `get` is this try / except one call further down) and one dict lookup: what a bare read costs"""
    try:
        v = _environ[name]
    except KeyError:
        return _UNSET[name]             # a KeyError of its own for an unknown name
    kind = _KIND[name]
    if kind == "text" or kind == "raw":
        return v
    if kind == "flag":
        return bool(v)
    if not v:
        return None
    try:
        return int(v)
    except ValueError:
        raise ValueError(f"{name}={v!r} is not an integer") from None


def markdown():
    """the table as DESIGN.md section 7g prints it"""
    rows = ["| variable | kind | unset | takes effect | read by | meaning |", "|---|---|---|---|---|---|"]
    for k in KNOBS.values():
        unset = {"flag": "off", "int": "none"}.get(k.kind) or (f"`{k.default}`" if k.default else "empty")
        rows.append(f"| `{k.name}` | {k.kind} | {unset} | {k.effect} | `{k.reader}` | {k.doc} |")
    return "\n".join(rows)


if __name__ == "__main__":
    print(markdown())
