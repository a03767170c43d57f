"""Records the public surface of ``bnn_amd.hipops`` into ``hipops_api.json`` (name -> ``str(inspect.signature(...))``):
run at the commit whose signatures are to be kept, ``python tests/golden/make_hipops_api.py``."""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "binary-networks-pytorch_amd"))
from bnn_amd import hipops  # noqa: E402

api = {n: str(inspect.signature(o)) for n, o in sorted(vars(hipops).items())
       if not n.startswith("_") and (inspect.isfunction(o) or inspect.isclass(o)) and o.__module__ == hipops.__name__}
with open(os.path.join(HERE, "hipops_api.json"), "w") as f:
    json.dump(api, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(api), "names")
