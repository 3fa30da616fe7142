"""Public names of the package (what ``from py_numpy_renderer_amd import *`` gives)."""
from .constants import PROJECTION_TYPE, SUBSYSTEM, SYSTEM
from .core import Accumulation, AmbientOcclusion, Bloom, Camera, DepthOfField, Layers, Light, LightShafts, Model, Morph, MotionBlur, Scene, Skin, TemporalAA, TextureMaps, ToneMap
from .cube_map import CubeMap
from .lightning import Lightning
from .materials import Material
from .triangular import Errors
from .transformation import rotate_xyz, scale, translation

__all__ = ["Errors", "CubeMap", "Accumulation", "AmbientOcclusion", "Bloom", "Camera", "DepthOfField", "Layers", "Light", "LightShafts", "Model", "Morph", "MotionBlur", "Scene", "Skin", "TemporalAA", "TextureMaps", "ToneMap", "Material",
           "Lightning", "PROJECTION_TYPE", "SUBSYSTEM", "SYSTEM", "scale", "translation", "rotate_xyz"]
