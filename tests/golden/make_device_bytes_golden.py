"""Record tests/golden/device_bytes.json: sgm_device_bytes of the handles of
tests/device_bytes_recipe.py, on the GPU.  Run it on the commit BEFORE a change
to sgm_create (the file pins what that commit allocated), with its library
built:

  python tests/golden/make_device_bytes_golden.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import device_bytes_recipe as recipe  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "device_bytes.json")
values = {name: recipe.measure(name) for name in recipe.CASES}
with open(out, "w") as f:
    json.dump(values, f, indent=1)
    f.write("\n")
print(json.dumps(values))
