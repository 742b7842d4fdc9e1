"""The argument stage of the drop-in CLI as one table: what `photonmap` answers to a command line
before it opens a device (tests/test_cli_arguments.py runs it).

A row is argv's tail after `missing.scn o.png` (both in a temporary directory, written `{tmp}`
here, and neither exists), the environment variables set for the run, and what the CLI did: its
exit code and its complete stderr, or PASSES for a command line that the argument stage lets
through. What fails next then differs between machines (the device on one without a GPU, the
missing scene file on one with), so such a row stands for: exit 255, and none of REFUSAL_TEXTS in
stderr. stdout is empty in every row, and no row leaves a file behind.

The answers were recorded, not written: from the `photonmap` binary of the commit before the
CLI's source was split into stages (5847c4e), built by its own Makefile on a machine without a
GPU, run once per row in a fresh directory holding make_files()'s files with GI_DEVICE and
GI_DEVICES unset, the directory's name replaced by `{tmp}`. The rows of the eight
tests/test_cli*.py files are all here; "two faults at once" pins the order in which the stage tests
things (the numbers are the steps of photonmap.cpp's ParseCommandLine), which is behaviour that a
later flag must not move by accident.
"""
import collections
import os
import struct
import subprocess

Case = collections.namedtuple("Case", "tail want env head", defaults=({}, None))
PASSES = None
REFUSAL_TEXTS = ("Invalid program argument", "Usage:", "not with", "views file", "-load_accum file")

CAM = "0.95 0.80 -1.2 -0.30 -0.20 1 0.1 1 0.05 0.40".split()
W, H = 24, 16


def _accum(w=W, h=H, passes_done=2, count=8, magic=b"GIACC01\n"):
    """A -load_accum file (photonmap.cpp AccumFile): header, W*H*6 doubles, W*H int64 counts."""
    npix = w * h
    return (struct.pack("<8siiq8s", magic, w, h, passes_done, b"\0" * 8)
            + struct.pack(f"<{npix * 6}d", *[0.25] * (npix * 6)) + struct.pack(f"<{npix}q", *[count] * npix))


def _views(*lines):
    return ("\n".join(lines) + "\n").encode()


_A = " ".join(CAM)
_B = " ".join(["1.1"] + CAM[1:])
FILES = {
    "views.txt": _views("# two cameras", _A, "", "  " + _B),
    "one.txt": _views("0.556 0.546 -1.6  0 0 1  0 1 0  0.329"),
    "nine.txt": _views(_A, "# a comment", " ".join(CAM[:9])),
    "eleven.txt": _views(_A + " 7"),
    "letter.txt": _views(_A.replace("1", "x", 1)),
    "empty.txt": _views("# nothing", ""),
    "good.acc": _accum(),
    "short_header.acc": _accum()[:20],
    "short_body.acc": _accum()[:-8],
    "long_body.acc": _accum() + b"\0",
    "magic.acc": _accum(magic=b"GIACC02\n"),
    "size.acc": _accum(16, 24),
    "negative.acc": _accum()[:-8] + struct.pack("<q", -1),
    "negative_passes.acc": _accum(passes_done=-1),
}
FILE_NAMES = tuple(FILES)


def make_files(tmp):
    for name, data in FILES.items():
        with open(os.path.join(str(tmp), name), "wb") as f:
            f.write(data)


def run_case(binary, tmp, tail, env=None, head=None):
    """The CLI on one row, in tmp (which holds make_files()'s files)."""
    tmp = str(tmp)
    if head is None:
        head = ["{tmp}/missing.scn", "{tmp}/o.png"]
    clean = {k: v for k, v in os.environ.items() if k not in ("GI_DEVICE", "GI_DEVICES")}
    clean.update(env or {})
    argv = [binary] + [a.replace("{tmp}", tmp) for a in list(head) + list(tail)]
    return subprocess.run(argv, capture_output=True, text=True, timeout=120, env=clean, cwd=tmp)


INVALID = "Invalid program argument: "
ONE_DEVICE = ("-passes, -noise, -exposure, -white, -radiance, -vdenoise and -views render on one device: "
              "not with -gpus 2\n")
ONE_VIEW = ("-layers takes whole-frame passes of one view: not with -adaptive, -views, -progressive, "
            "-save_accum or -load_accum\n")

CASES = [
    # ---- gi_parse_args's own refusals (tests/test_cli.py)
    Case([], (255, "Usage: photonmap inputscenefile outputimagefile [-FLAGS]\n"), head=[]),
    Case([],
         (255, "Usage: photonmap inputscenefile outputimagefile [-FLAGS]\n"), head=["only_scene.scn"]),
    Case(["b.png", "-bogus"], (1, INVALID + "-bogus"), head=["a.scn"]),
    Case(["b.png", "extra"], (1, INVALID + "extra"), head=["a.scn"]),
    Case(["-v", "b.png", "-no_shadow", "-nonsense", "3"],
         (1, INVALID + "-nonsense"), head=["a.scn"]),
    Case(["-bogus"], (1, INVALID + "-bogus")),
    # ---- -camera (tests/test_cli_camera.py)
    Case(["-camera", "1", "2", "3"], (1, INVALID + "-camera")),
    Case(["-camera"], (1, INVALID + "-camera")),
    Case(["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "9"], (1, INVALID + "-camera")),
    Case(["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "x", "0.3"], (1, INVALID + "-camera")),
    Case(["-camera", "1", "2", "3", "4", "5", "6", "7", "8", "9", "0.3f"],
         (1, INVALID + "-camera")),
    Case(["-v", "-camera", "1", "2", "3", "-no_shadow", "4", "5", "6", "7", "8", "9"],
         (1, INVALID + "-camera")),
    Case(["-aa", "0", "-camera"] + CAM + ["-no_shadow"], PASSES),
    Case(["-camera"] + CAM + ["-bogus"], (1, INVALID + "-bogus")),
    Case(["-camera"] + CAM + ["-camera", "1", "2"], (1, INVALID + "-camera")),
    Case(["-camera", "1", "2", "-camera"] + CAM, (1, INVALID + "-camera")),
    Case(["-camera", "nan"] + CAM[1:],
         PASSES),
    # ---- -denoise (tests/test_cli_denoise.py)
    Case(["-denoise"], (1, INVALID + "-denoise")),
    Case(["-aa", "0", "-denoise"], (1, INVALID + "-denoise")),
    Case(["-denoise", "x"], (1, INVALID + "-denoise")),
    Case(["-denoise", "2.5"], (1, INVALID + "-denoise")),
    Case(["-denoise", "3x"], (1, INVALID + "-denoise")),
    Case(["-denoise", "0"], (1, INVALID + "-denoise")),
    Case(["-denoise", "9"], (1, INVALID + "-denoise")),
    Case(["-denoise", "-1"], (1, INVALID + "-denoise")),
    Case(["-denoise", "-no_shadow"], (1, INVALID + "-denoise")),
    Case(["-denoise", "5", "-v", "-denoise", "12"], (1, INVALID + "-denoise")),
    Case(["-denoise", "x", "-denoise", "3"], (1, INVALID + "-denoise")),
    Case(["-aa", "0", "-denoise", "1", "-no_shadow"], PASSES),
    Case(["-aa", "0", "-denoise", "5", "-no_shadow"], PASSES),
    Case(["-aa", "0", "-denoise", "8", "-no_shadow"], PASSES),
    Case(["-denoise", "1", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-denoise", "5", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-denoise", "8", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-denoise", "3", "-camera"] + CAM + ["-bogus"], (1, INVALID + "-bogus")),
    Case(["-camera"] + CAM[:4] + ["-denoise", "3"] + CAM[4:],
         (1, INVALID + "-camera")),
    # ---- -vdenoise (tests/test_cli_vdenoise.py)
    Case(["-vdenoise", "0"], (1, INVALID + "-vdenoise")),
    Case(["-vdenoise", "9"], (1, INVALID + "-vdenoise")),
    Case(["-vdenoise"], (1, INVALID + "-vdenoise")),
    Case(["-vdenoise", "2.5"], (1, INVALID + "-vdenoise")),
    Case(["-vdenoise", "3", "-denoise", "3"], (1, INVALID + "-vdenoise")),
    Case(["-denoise", "3", "-passes", "2", "-vdenoise", "3"], (1, INVALID + "-vdenoise")),
    Case(["-vdenoise", "9", "-vdenoise", "2"], (1, INVALID + "-vdenoise")),
    Case(["-aa", "1", "-vdenoise", "3", "-no_shadow"], PASSES),
    Case(["-vdenoise", "3", "-gpus", "2"], (255, ONE_DEVICE)),
    # ---- -passes, -noise, -exposure, -white, -radiance (tests/test_cli_radiance.py)
    Case(["-passes"], (1, INVALID + "-passes")),
    Case(["-passes", "x"], (1, INVALID + "-passes")),
    Case(["-passes", "2.5"], (1, INVALID + "-passes")),
    Case(["-passes", "0"], (1, INVALID + "-passes")),
    Case(["-passes", "4097"], (1, INVALID + "-passes")),
    Case(["-passes", "3", "-v", "-passes", "-1"], (1, INVALID + "-passes")),
    Case(["-passes", "x", "-passes", "3"], PASSES),
    Case(["-passes", "2", "-passes"], (1, INVALID + "-passes")),
    Case(["-noise", "x", "-noise", "0.1"], PASSES),
    Case(["-aa", "0", "-noise"], (1, INVALID + "-noise")),
    Case(["-noise", "-0.5"], (1, INVALID + "-noise")),
    Case(["-noise", "nan"], (1, INVALID + "-noise")),
    Case(["-noise", "-no_shadow"], (1, INVALID + "-noise")),
    Case(["-exposure", "0"], (1, INVALID + "-exposure")),
    Case(["-exposure", "-2"], (1, INVALID + "-exposure")),
    Case(["-exposure", "inf"], (1, INVALID + "-exposure")),
    Case(["-exposure", "1x"], (1, INVALID + "-exposure")),
    Case(["-white", "-1"], (1, INVALID + "-white")),
    Case(["-white"], (1, INVALID + "-white")),
    Case(["-radiance"], (1, INVALID + "-radiance")),
    Case(["-radiance", "f.png"], (1, INVALID + "-radiance")),
    Case(["-radiance", "noextension"], (1, INVALID + "-radiance")),
    Case(["-passes", "3", "-aa", "0", "-noise", "0.01", "-exposure", "0.5", "-no_shadow", "-white", "4",
          "-radiance", "{tmp}/f.hdr"],
         PASSES),
    Case(["-passes", "3", "-aa", "0", "-noise", "0.01", "-exposure", "0.5", "-no_shadow", "-white", "4",
          "-radiance", "{tmp}/f.hdr", "-bogus"],
         (1, INVALID + "-bogus")),
    Case(["-passes", "4096", "-radiance", "{tmp}/f.pfm"], PASSES),
    Case(["-passes", "2", "-gpus", "2"], (255, ONE_DEVICE)),
    # ---- -adaptive [TILE] (tests/test_cli_adaptive.py)
    Case(["-adaptive"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "8"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "7"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "3"], (1, INVALID + "-adaptive")),
    Case(["-passes", "4", "-adaptive", "8", "-exposure", "2"], (1, INVALID + "-adaptive")),
    Case(["-noise", "0.02", "-adaptive", "3"], (1, INVALID + "-adaptive")),
    Case(["-noise", "0.02", "-adaptive", "65"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "-1", "-noise", "0.02"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "8", "-noise", "0.02", "-adaptive", "2"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "-noise", "0.1", "-adaptive", "70"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "70", "-noise", "0.1", "-adaptive"], (1, INVALID + "-adaptive")),
    Case(["-adaptive", "-noise", "0.02"], PASSES),
    Case(["-noise", "0.02", "-aa", "0", "-adaptive"], PASSES),
    Case(["-adaptive", "16", "-noise", "0.02", "-no_shadow"], PASSES),
    Case(["-noise", "0.02", "-adaptive", "-no_shadow"], PASSES),
    Case(["-noise", "0.02", "-adaptive", "4"], PASSES),
    Case(["-noise", "0.02", "-adaptive", "64"], PASSES),
    Case(["-noise", "0.02", "-adaptive", "16", "-adaptive"], PASSES),
    Case(["-noise", "0.02", "-adaptive", "8.5"], (1, INVALID + "8.5")),
    Case(["-noise", "0.02", "-adaptive", "-gpus", "2"], (255, ONE_DEVICE)),
    # ---- -save_accum, -load_accum (tests/test_cli_accum_state.py)
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/missing.acc"],
         (255, "Unable to read -load_accum file {tmp}/missing.acc: cannot open it\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/short_header.acc"],
         (255, "Unable to read -load_accum file {tmp}/short_header.acc: shorter than its header\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/short_body.acc"],
         (255, "Unable to read -load_accum file {tmp}/short_body.acc: shorter than its 21536 bytes\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/long_body.acc"],
         (255, "Unable to read -load_accum file {tmp}/long_body.acc: longer than its 21536 bytes\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/magic.acc"],
         (255, "Unable to read -load_accum file {tmp}/magic.acc: not an accumulator file (bad magic)\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/size.acc"],
         (255, "Unable to read -load_accum file {tmp}/size.acc: it holds 16 x 24 pixels, -resolution is 24 x 16\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/negative.acc"],
         (255, "Unable to read -load_accum file {tmp}/negative.acc: negative sample count\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/negative_passes.acc"],
         (255, "Unable to read -load_accum file {tmp}/negative_passes.acc: negative pass count\n")),
    Case(["-load_accum", "{tmp}/good.acc"],
         (255, "Unable to read -load_accum file {tmp}/good.acc: it holds 24 x 16 pixels, -resolution is 1024 x 1024\n")),
    Case(["-resolution", "24", "16", "-save_accum", "{tmp}/s.acc", "-views", "{tmp}/one.txt"],
         (255, INVALID + "-views (not with -save_accum or -load_accum)\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/good.acc", "-views", "{tmp}/one.txt"],
         (255, INVALID + "-views (not with -save_accum or -load_accum)\n")),
    Case(["-resolution", "24", "16", "-save_accum", "{tmp}/s.acc", "-gpus", "2"],
         (255, ONE_DEVICE)),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/good.acc", "-gpus", "2"],
         (255, ONE_DEVICE)),
    Case(["-resolution", "24", "16", "-save_accum"], (1, INVALID + "-save_accum")),
    Case(["-resolution", "24", "16", "-load_accum"], (1, INVALID + "-load_accum")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/good.acc", "-save_accum", "{tmp}/s.acc"],
         PASSES),
    # ---- -progressive A (tests/test_cli_progressive.py renders with it)
    Case(["-progressive"], (1, INVALID + "-progressive")),
    Case(["-progressive", "0"], (1, INVALID + "-progressive")),
    Case(["-progressive", "1"], (1, INVALID + "-progressive")),
    Case(["-progressive", "x"], (1, INVALID + "-progressive")),
    Case(["-progressive", "nan"], (1, INVALID + "-progressive")),
    Case(["-progressive", "0.5", "-adaptive", "-noise", "0.1"],
         (1, INVALID + "-progressive (not with -adaptive)")),
    Case(["-progressive", "0.5", "-views", "{tmp}/views.txt"],
         (255, INVALID + "-progressive (not with -views)\n")),
    Case(["-progressive", "0.5", "-cache"], (255, INVALID + "-progressive (not with -cache)\n")),
    Case(["-progressive", "0.5", "-gpus", "2"],
         (255, "-progressive renders on one device: not with -gpus 2\n")),
    Case(["-progressive", "0.5", "-passes", "2"], PASSES),
    Case(["-progressive", "0.7", "-noise", "0.01", "-save_accum", "{tmp}/s.acc"], PASSES),
    # ---- -layers PREFIX (tests/test_cli_layers.py)
    Case(["-layers", "{tmp}/p", "-adaptive", "-noise", "0.05"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-views", "v.txt"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-progressive", "0.7"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-save_accum", "a.acc"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-load_accum", "a.acc"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-gpus", "2"],
         (1, "-layers renders on one device: not with -gpus 2\n")),
    Case(["-layers", "{tmp}/p", "-passes", "2", "-gpus", "2"],
         (1, "-layers renders on one device: not with -gpus 2\n")),
    Case(["-layers"], (1, INVALID + "-layers")),
    Case(["-layers", "{tmp}/p"], PASSES),
    Case(["-layers", "{tmp}/p", "-passes", "2", "-vdenoise", "2"], PASSES),
    Case(["-layers", "{tmp}/p", "-denoise", "2"], PASSES),
    # ---- -views FILE, -history H (tests/test_cli_reproject.py)
    Case(["-views", "{tmp}/nothing.txt"], (255, "Unable to open views file {tmp}/nothing.txt\n")),
    Case(["-passes", "2", "-views"], (255, INVALID + "-views\n")),
    Case(["-views", "{tmp}/nine.txt"],
         (255, "Unable to read views file {tmp}/nine.txt: line 3 is not ten numbers\n")),
    Case(["-views", "{tmp}/eleven.txt"],
         (255, "Unable to read views file {tmp}/eleven.txt: line 1 is not ten numbers\n")),
    Case(["-views", "{tmp}/letter.txt"],
         (255, "Unable to read views file {tmp}/letter.txt: line 1 is not ten numbers\n")),
    Case(["-views", "{tmp}/empty.txt"],
         (255, "Unable to read views file {tmp}/empty.txt: no camera in it\n")),
    Case(["-views", "{tmp}/views.txt", "-history", "1"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-history", "0"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-history", "-3"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-history", "x"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-history", "2.5"], (255, INVALID + "-history\n")),
    Case(["-history", "8"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-history"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-denoise", "3"],
         (255, INVALID + "-views (not with -denoise)\n")),
    Case(["-views", "{tmp}/views.txt", "-gpus", "2"], (255, ONE_DEVICE)),
    Case(["-views", "{tmp}/views.txt", "-aa", "0", "-history", "16", "-vdenoise", "2"], PASSES),
    Case(["-views", "{tmp}/views.txt", "-history", "2"], PASSES),
    Case(["-views", "{tmp}/views.txt"], PASSES),
    Case(["-views", "{tmp}/nothing.txt", "-views", "{tmp}/views.txt"], PASSES),
    Case(["-views", "{tmp}/views.txt", "-views", "{tmp}/nothing.txt"],
         (255, "Unable to open views file {tmp}/nothing.txt\n")),
    # ---- two faults at once: the one that is tested first is reported
    Case(["-camera", "1", "2", "-denoise", "0"], (1, INVALID + "-camera")),
    Case(["-denoise", "0", "-vdenoise", "0"], (1, INVALID + "-denoise")),
    Case(["-vdenoise", "3", "-denoise", "3", "-passes", "0"], (1, INVALID + "-vdenoise")),
    Case(["-denoise", "0", "-passes", "0"], (1, INVALID + "-denoise")),
    Case(["-adaptive", "3", "-passes", "0"], (1, INVALID + "-adaptive")),
    Case(["-passes", "0", "-noise", "-1"], (1, INVALID + "-passes")),
    Case(["-noise", "-1", "-exposure", "0"], (1, INVALID + "-noise")),
    Case(["-exposure", "0", "-white", "-1"], (1, INVALID + "-exposure")),
    Case(["-white", "-1", "-radiance", "f.png"], (1, INVALID + "-white")),
    Case(["-radiance", "f.png", "-save_accum"], (1, INVALID + "-radiance")),
    Case(["-load_accum", "-save_accum"], (1, INVALID + "-save_accum")),
    Case(["-load_accum", "{tmp}/missing.acc", "-progressive"], (1, INVALID + "-progressive")),
    Case(["-progressive", "2", "-adaptive"], (1, INVALID + "-progressive")),
    Case(["-progressive", "0.5", "-adaptive"], (1, INVALID + "-progressive (not with -adaptive)")),
    Case(["-adaptive", "-passes", "2"], (1, INVALID + "-adaptive")),
    Case(["-passes", "0", "-layers"], (1, INVALID + "-passes")),
    Case(["-adaptive", "-layers"], (1, INVALID + "-adaptive")),
    Case(["-views", "-layers"], (1, INVALID + "-layers")),
    Case(["-history", "-views"], (255, INVALID + "-views\n")),
    Case(["-layers", "{tmp}/p", "-adaptive", "-views", "nothing"], (1, INVALID + "-adaptive")),
    Case(["-layers", "{tmp}/p", "-adaptive", "-noise", "0.1", "-views"],
         (255, INVALID + "-views\n")),
    Case(["-layers", "{tmp}/p", "-progressive", "0.5", "-history"], (255, INVALID + "-history\n")),
    Case(["-layers", "{tmp}/p", "-views", "{tmp}/views.txt", "-history", "1"], (1, ONE_VIEW)),
    Case(["-views", "{tmp}/views.txt", "-history", "1", "-denoise", "2"],
         (255, INVALID + "-history\n")),
    Case(["-history", "4", "-save_accum", "{tmp}/s.acc"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/views.txt", "-save_accum", "{tmp}/s.acc", "-progressive", "0.5"],
         (255, INVALID + "-views (not with -save_accum or -load_accum)\n")),
    Case(["-views", "{tmp}/views.txt", "-progressive", "0.5", "-denoise", "2"],
         (255, INVALID + "-progressive (not with -views)\n")),
    Case(["-views", "{tmp}/nothing.txt", "-denoise", "2"],
         (255, INVALID + "-views (not with -denoise)\n")),
    Case(["-history", "4", "-bogus"], (255, INVALID + "-history\n")),
    Case(["-views", "{tmp}/nothing.txt", "-bogus"],
         (255, "Unable to open views file {tmp}/nothing.txt\n")),
    Case(["-views", "{tmp}/views.txt", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-passes", "2", "-gpus", "2", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-layers", "{tmp}/p", "-gpus", "2", "-bogus"], (1, INVALID + "-bogus")),
    Case(["-layers", "{tmp}/p", "-gpus", "2", "-progressive", "0.5"], (1, ONE_VIEW)),
    Case(["-layers", "{tmp}/p", "-gpus", "2", "-vdenoise", "3"],
         (1, "-layers renders on one device: not with -gpus 2\n")),
    Case(["-progressive", "0.5", "-cache", "-gpus", "2"],
         (255, INVALID + "-progressive (not with -cache)\n")),
    Case(["-progressive", "0.5", "-gpus", "2", "-passes", "2"],
         (255, "-progressive renders on one device: not with -gpus 2\n")),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/magic.acc", "-gpus", "2"],
         (255, ONE_DEVICE)),
    Case(["-resolution", "24", "16", "-load_accum", "{tmp}/magic.acc", "-progressive", "0.5", "-cache"],
         (255, INVALID + "-progressive (not with -cache)\n")),
    # ---- the device set is read from the environment too
    Case(["-passes", "2"], (255, ONE_DEVICE), env={"GI_DEVICES": "0,0"}),
    Case(["-passes", "2"], PASSES, env={"GI_DEVICES": ""}),
    Case(["-passes", "2"], PASSES, env={"GI_DEVICES": "0"}),
    Case(["-passes", "2"], PASSES, env={"GI_DEVICE": "0"}),
    Case(["-layers", "{tmp}/p"],
         (1, "-layers renders on one device: not with -gpus 3\n"), env={"GI_DEVICES": "0,1,2"}),
    Case(["-progressive", "0.5"],
         (255, "-progressive renders on one device: not with -gpus 2\n"), env={"GI_DEVICES": "0,0"}),
    Case(["-gpus", "2", "-passes", "2"], PASSES, env={"GI_DEVICES": "0"}),
]
