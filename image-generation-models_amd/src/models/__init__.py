"""Models with the reference's surface.  Import them from their modules (`src.models.ddpm`, `src.models.factor_vae`, ...), as the
configs' `_target_`s do; `src.models.FactorVAE` and `src.models.AAE` are resolved lazily (the networks import `src.models.ddpm`, so
nothing may be imported here at package load); `src.models.GAN`, `src.models.InfoGAN`, `src.models.AGE`, `src.models.VAEGAN` and `src.models.BiGAN` (the module of that name, which holds the class) likewise."""


def __getattr__(name):
    if name == "FactorVAE":
        from .factor_vae import FactorVAE
        return FactorVAE
    if name == "AAE":
        from .aae import AAE
        return AAE
    if name == "GAN":
        from .gan import GAN
        return GAN
    if name == "InfoGAN":
        from .info_gan import InfoGAN
        return InfoGAN
    if name == "AGE":
        from .age import AGE
        return AGE
    if name == "VAEGAN":
        from .vae_gan import VAEGAN
        return VAEGAN
    if name == "BiGAN":
        import importlib
        return importlib.import_module(".BiGAN", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
