"""Drop-in import surface of the module the reference's `detector: sam` path imports (anime_3dkenburns/kenburns_effect.py:851
`from sam import apply_sam`; the reference does not vendor it): resolves to the MI355X implementation (cartoonsegmentation_amd.sam)."""
from cartoonsegmentation_amd.sam import Sam, apply_sam  # noqa: F401
