"""The comparison baselines whose training loops live in the reference's baselines/ package, on the HIP path (SCRUB: SCRUBtrain.py; LwF, DER /
DER++ and FDR: Lwftrain.py, DERtrain.py, FDRtrain.py over the shared loop of _distill.py; LIRF: LIRFtrain.py)."""
