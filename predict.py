"""Label-map files from scans with the exported model (see unet_distributed_amd/predict.py)."""
from unet_distributed_amd.predict import main

if __name__ == "__main__":
    main()
