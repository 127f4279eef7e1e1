"""Regenerates tests/golden/reference_outputs.json: what the reference's OWN code outputs for the inputs of tests/test_reference_build.py --
its OBJ importer, frame, CSG, exporters and header helpers, run through oracle/_ref (`make -C oracle _ref`, which needs the reference tree).
Each value comes from the record_* function of that test module the test compares with."""
import importlib.util, json, os, pathlib, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O
from cuda_mesh_voxelization_amd import build
if O.build_ref() is None:
    sys.exit("oracle/_ref is not built: make -C oracle _ref (needs the reference tree)")
spec = importlib.util.spec_from_file_location("test_reference_build", os.path.join(ROOT, "tests", "test_reference_build.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)
cli = build.build_cli()
out = {"import": {}, "frame": {}, "csg": {}, "gpu_csg": {}, "exports": {}, "cli_exports": {}}
with tempfile.TemporaryDirectory() as tmp:
    def sub(name):
        d = pathlib.Path(tmp) / name
        d.mkdir()
        return d
    for name in T.ASSETS:
        out["import"][name] = T.record_import(name, str(sub("import_" + name)))
    out["import_bunny_x3"] = T.record_import_bunny_x3(str(sub("bunny_x3")))
    for names, n in T.FRAMES:
        out["frame"]["%s@%d" % ("+".join(names), n)] = T.record_frame(names, n)
    for op in T.CSG_OPS:
        out["csg"][str(op)] = T.record_csg(op, str(sub("csg%d" % op)))
        out["gpu_csg"][str(op)] = T.record_gpu_csg(op, str(sub("gpu_csg%d" % op)))
    for name, n in T.EXPORTS:
        out["exports"]["%s@%d" % (name, n)] = T.record_exports(name, n, str(sub("exports_%s_%d" % (name, n))))
    # the grid and sdf of `vpcli -t 0`: the CPU path, which -t 3 and the GPU path (-t 2) equal bit for bit
    for name, n in dict.fromkeys(T.CLI_EXPORTS + T.GPU_EXPORTS):
        out["cli_exports"]["%s@%d" % (name, n)] = T.record_cli_exports(cli, sub("cli_%s_%d" % (name, n)), name, n, 0)
    out["vector_ops"] = T.record_vector_ops(str(sub("vector_ops")))
    out["helpers"] = T.record_helpers()
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "reference_outputs.json"), "w"), indent=1)
