* common-source amplifier: channel noise of M1 and the noise of RD at the drain, input-referred through VIN
VDD vdd 0 DC 3
VIN g 0 DC 0.9 AC 1
RD vdd d 5k
CL d 0 1p
M1 d g 0 n 10e-6 1e-6 2
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.05 CJ0 4.0e-14
.noise v(d) vin dec 10 1k 1g
