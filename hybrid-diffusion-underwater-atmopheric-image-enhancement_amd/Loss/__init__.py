"""The reference's ``Loss`` package: the loss modules of the second tree that run on the HIP path."""
from .loss import MSSSIMLoss  # noqa: F401
