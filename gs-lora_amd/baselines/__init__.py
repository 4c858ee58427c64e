"""The comparison baselines whose training loops live in the reference's baselines/ package, on the HIP path (SCRUB: SCRUBtrain.py)."""
